"""GPU: the glue launchers that run on every step, one operator call per case through the C-ABI test entry points d4_rmsnorm / d4_layernorm_rows /
d4_gather_space_double_norm / d4_assemble_tokens / d4_cvt_rows_bf16 / d4_cvt_bf16 / d4_cvt_pad_bf16 / d4_cvt_transpose_bf16 / d4_colsum /
d4_colsum_batch / d4_rmsnorm_bwd / d4_adamw_clip / d4_splitk_reduce / d4_mean_tokens / d4_hl_gauss_scalar_strided / d4_euler_step_rows / d4_unary_rows /
d4_copy_rows / d4_pad_cols / d4_video_patches / d4_cache_transfer / d4_cunembed / d4_coord_grid / d4_pack_tokens / d4_fold_rows /
d4_swiglu_pack_rows / d4_build_latent_input / d4_prep_eval_inputs / d4_layernorm_silu_bwd / d4_silu_bwd / d4_swiglu / d4_multi_copy / d4_zero_pad_cols, each against the plain reference of tests/glue_ref.py.

A case (tests/glue_cases.py) asserts
  * (the form: where a launcher chooses between kernels a case names the kernel its sizes and alignments select; the host test checks the name
    against the launcher's rule, and the case asserts here that its pointers have the alignment that rule assumes (16 bytes for a register / float4
    form, 4 bytes past it for an `off` case), so every form of every launcher runs — the library itself does not report the choice);
  * the values: max |out - float64| <= BOUND[family] x max |float64| for the numeric families; bit for bit for the bf16 images (torch's
    round-to-nearest-even), the token assembly (copies; the action token's float32 sum in the kernel's order, the continuous part by fma), the
    index permutations and copies (torch indexing of the logical tensors) and colsum_batch against the single colsum launch of the same matrix;
  * untouched memory: every operand and output lies between NaN guards with NaN in the gaps of its padded rows; whatever the operation must
    not write is still NaN afterwards, and a read past a row poisons the output.
The last test prints each family's worst error as a fraction of its bound.

Tolerance (glue_cases.py): E32 = float32 against float64 evaluation of the same reference on the CPU (reductions added term after term), worst
case of the family, recorded with 25 % headroom; the GPU bound is 8 x E32, relative to the output's max-abs:
    family           measured E32   recorded E32   bound (8 x)
    rmsnorm_rows     1.33e-7        1.7e-7         1.4e-6
    layernorm_rows   6.72e-6        8.4e-6         6.7e-5
    gather_space     1.53e-7        1.9e-7         1.5e-6
    rmsnorm_bwd      1.34e-7        1.7e-7         1.4e-6
    colsum           3.53e-6        4.4e-6         3.5e-5
    adamw            7.23e-7        9.0e-7         7.2e-6
    adamw_wide       4.95e-4        6.2e-4         5.0e-3
    splitk_reduce    1.42e-7        1.8e-7         1.4e-6
    mean_tokens      1.09e-7        1.4e-7         1.1e-6
    hl_gauss_scalar  1.02e-7        1.3e-7         1.0e-6
    euler_step       5.97e-8        7.5e-8         6.0e-7
    unary            4.23e-8        5.3e-8         4.2e-7      (silu_rows, tanh_rows)
    build_latent_input 4.97e-8      6.2e-8         5.0e-7      (w = 0.3, 0.7; w = 0 and 1 are copies, bit for bit)
    silu_bwd         6.72e-7        8.4e-7         6.7e-6
    layernorm_silu_bwd 2.68e-6      3.4e-6         2.7e-5
    swiglu           1.53e-7        1.9e-7         1.5e-6      (swiglu_fwd, swiglu_bwd)"""
import ctypes as C

import pytest
import torch

import glue_cases as GC
import glue_ref as G
from dreamer4_amd import _lib
from test_gpu_attn_cores import DEV, GUARD, Buf, bits, check_image, stream

pytestmark = pytest.mark.gpu

WORST = {}                       # family -> (error / bound, what)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def note(family, name, err):
    bound = GC.BOUND[family]
    print(f'{family} {name}: err {err:.3e} (bound {bound:.3e})')
    if family not in WORST or err / bound > WORST[family][0]:
        WORST[family] = (err / bound, f'{name}: {err:.3e} of {bound:.3e}')


def rows_in(x, ld, off=0):
    """x [rows, cols] (CPU) as rows of leading dimension ld, NaN in the gaps -> uploaded Buf"""
    rows, cols = x.shape
    b = Buf(rows * ld, off, dtype=x.dtype)
    b.view((rows, cols), (ld, 1)).copy_(x)
    return b.upload()


def flat_in(x, off=0):
    return rows_in(x.reshape(1, -1), x.numel(), off)


def out_buf(size, off=0, dtype=torch.float32):
    return Buf(size, off, dtype).upload()


def aligned(form_is_vec, *ptrs, by=16):
    """The alignment the launcher's rule assumes of a case's pointers: all of them on `by` bytes where the case names a register / float4 form, the
    last one off it where the case is scalar by its `off`."""
    vals = [p.value if isinstance(p, C.c_void_p) else p for p in ptrs]
    if form_is_vec:
        assert all(v % by == 0 for v in vals), f'a pointer of a vector-form case is not {by}-byte aligned: the scalar kernel would run'
    else:
        assert vals[-1] % by == 4, 'the offset pointer of a scalar-by-alignment case is aligned: the vector kernel would run'


def image(buf, ref, ld=None, dtype=torch.float64):
    """The expected content of `buf`, guards included: `ref` [rows, cols] at leading dimension ld (a flat ref: as it is), NaN everywhere else."""
    w = Buf(buf.size, buf.off, buf.dtype).host.to(dtype)
    ref = ref.reshape(1, -1) if ld is None else ref
    w.as_strided(ref.shape, (ld or ref.shape[1], 1), GUARD + buf.off).copy_(ref)
    return w


def check_exact(buf, want):
    """bit for bit where `want` holds a value, untouched (NaN) where it holds NaN"""
    got = buf.dev.cpu()
    keep = want.isnan()
    assert got[keep].isnan().all(), f'{int((~got[keep].isnan()).sum())} elements written that the operation must not touch'
    g, w = bits(got[~keep]), bits(want[~keep])
    assert torch.equal(g, w), f'{int((g != w).sum())} of {w.numel()} elements differ in their bits'


# ------------------------------------------------------------------------------------------------------------------- row norms
@pytest.mark.parametrize('c', GC.RMSNORM, ids=[c['name'] for c in GC.RMSNORM])
def test_rmsnorm_rows(lib, c):
    d = GC.rmsnorm_inputs(c)
    ld = c['D'] + c['pad']
    x = rows_in(d['x'], ld)
    gamma = None if d['gamma'] is None else flat_in(d['gamma'], 1 if c['gamma'] == 'off' else 0)
    y = out_buf(c['rows'] * ld)
    if c['form'] == 'vec' or c['gamma'] == 'off':
        aligned(c['form'] == 'vec', x.ptr, y.ptr, *([gamma.ptr] if gamma else []))
    _lib.check(lib.d4_rmsnorm(x.ptr, ld, gamma.ptr if gamma else None, y.ptr, ld, c['rows'], c['D'], c['eps'], stream()))
    torch.cuda.synchronize()
    note('rmsnorm_rows', c['name'], check_image(y.dev, image(y, GC.rmsnorm_expect(c, d)[0], ld), GC.BOUND['rmsnorm_rows']))


@pytest.mark.parametrize('c', GC.LAYERNORM, ids=[c['name'] for c in GC.LAYERNORM])
def test_layernorm_rows(lib, c):
    d = GC.layernorm_inputs(c)
    ldx, ldy = c['D'] + c['pad'], c['D'] + 2 * c['pad']
    x, g = rows_in(d['x'], ldx), flat_in(d['g'])
    b = None if d['b'] is None else flat_in(d['b'])
    y = out_buf(c['rows'] * ldy)
    _lib.check(lib.d4_layernorm_rows(x.ptr, ldx, g.ptr, b.ptr if b else None, y.ptr, ldy, c['rows'], c['D'], c['eps'], c['silu'], stream()))
    torch.cuda.synchronize()
    note('layernorm_rows', c['name'], check_image(y.dev, image(y, GC.layernorm_expect(c, d)[0], ldy), GC.BOUND['layernorm_rows']))


def test_layernorm_refuses_a_row_wider_than_its_registers(lib):
    x, g, y = flat_in(torch.ones(4097)), flat_in(torch.ones(4097)), out_buf(4097)
    with pytest.raises(_lib.D4Error, match='layernorm: row width 4097 > 4096'):
        _lib.check(lib.d4_layernorm_rows(x.ptr, 4097, g.ptr, None, y.ptr, 4097, 1, 4097, 1e-5, 0, stream()))
    with pytest.raises(_lib.D4Error, match='d4_layernorm_rows: bad arguments'):
        _lib.check(lib.d4_layernorm_rows(x.ptr, 63, g.ptr, None, y.ptr, 64, 1, 64, 1e-5, 0, stream()))
    torch.cuda.synchronize()
    assert y.dev.isnan().all(), 'a refused call wrote an output'


@pytest.mark.parametrize('c', GC.GATHER_SPACE, ids=[c['name'] for c in GC.GATHER_SPACE])
def test_gather_space_double_norm(lib, c):
    d = GC.gather_inputs(c)
    tokens = flat_in(d['tokens'], c['off'])
    g0, g1 = flat_in(d['g0']), flat_in(d['g1'])
    out = out_buf(c['frames'] * c['ns'] * c['D'])
    if c['form'] != 'generic' or c['off']:
        aligned(c['form'] != 'generic', out.ptr, g0.ptr, g1.ptr, tokens.ptr)
    _lib.check(lib.d4_gather_space_double_norm(tokens.ptr, out.ptr, g0.ptr, g1.ptr, c['frames'], c['S'], c['first'], c['D'], c['ns'], c['eps'], stream()))
    torch.cuda.synchronize()
    note('gather_space', c['name'], check_image(out.dev, image(out, GC.gather_expect(c, d)[0]), GC.BOUND['gather_space']))


def test_gather_space_refuses_rows_outside_the_frame(lib):
    t, g, out = flat_in(torch.ones(2 * 4 * 8)), flat_in(torch.ones(8)), out_buf(2 * 3 * 8)
    with pytest.raises(_lib.D4Error, match='d4_gather_space_double_norm: bad arguments'):
        _lib.check(lib.d4_gather_space_double_norm(t.ptr, out.ptr, g.ptr, g.ptr, 2, 4, 2, 8, 3, 1e-6, stream()))
    torch.cuda.synchronize()
    assert out.dev.isnan().all(), 'a refused call wrote an output'


@pytest.mark.parametrize('c', GC.RMSNORM_BWD, ids=[c['name'] for c in GC.RMSNORM_BWD])
def test_rmsnorm_bwd(lib, c):
    d = GC.rmsbwd_inputs(c)
    x, dxhat, gamma = flat_in(d['x']), flat_in(d['dxhat']), flat_in(d['gamma'])
    n = c['rows'] * c['D']
    tg, dx = out_buf(n), out_buf(n)
    _lib.check(lib.d4_rmsnorm_bwd(x.ptr, dxhat.ptr, gamma.ptr, tg.ptr, dx.ptr if c['dx'] else None, c['rows'], c['D'], c['eps'], stream()))
    torch.cuda.synchronize()
    ref_tg, ref_dx = GC.rmsbwd_expect(c, d)
    err = check_image(tg.dev, image(tg, ref_tg), GC.BOUND['rmsnorm_bwd'])
    if c['dx']:
        err = max(err, check_image(dx.dev, image(dx, ref_dx), GC.BOUND['rmsnorm_bwd']))
    else:
        assert dx.dev.isnan().all()
    note('rmsnorm_bwd', c['name'], err)


# ------------------------------------------------------------------------------------------------------------------- reductions
def colsum_call(lib, x, ld, rows, cols, scratch_floats=0):
    out = out_buf(cols)
    scratch = out_buf(scratch_floats) if scratch_floats else None
    _lib.check(lib.d4_colsum(x.ptr, ld, rows, cols, out.ptr, scratch.ptr if scratch else None, scratch_floats, stream()))
    torch.cuda.synchronize()
    if scratch:                                              # (the partial rows stay inside the scratch handed over)
        assert scratch.dev[:GUARD].isnan().all() and scratch.dev[GUARD + scratch_floats:].isnan().all()
    return out


@pytest.mark.parametrize('c', GC.COLSUM, ids=[c['name'] for c in GC.COLSUM])
def test_colsum(lib, c):
    d = GC.colsum_inputs(c)
    ld = c['cols'] + c['pad']
    out = colsum_call(lib, rows_in(d['x'], ld), ld, c['rows'], c['cols'], c['scratch'])
    note('colsum', c['name'], check_image(out.dev, image(out, GC.colsum_expect(c, d)[0]), GC.BOUND['colsum']))


@pytest.mark.parametrize('c', GC.COLSUM_BATCH, ids=[c['name'] for c in GC.COLSUM_BATCH])
def test_colsum_batch_is_the_single_launch_bit_for_bit(lib, c):
    mats = GC.colsum_batch_inputs(c)['mats']
    n = len(mats)
    lds = [x.shape[1] + c['pad'] for x in mats]
    xs = [rows_in(x, ld) for x, ld in zip(mats, lds)]
    outs = [out_buf(x.shape[1]) for x in mats]
    arr = lambda t, v: (t * n)(*v)
    _lib.check(lib.d4_colsum_batch(n, arr(C.c_void_p, [x.ptr.value for x in xs]), arr(C.c_int32, lds), arr(C.c_int32, [x.shape[0] for x in mats]),
                                   arr(C.c_int32, [x.shape[1] for x in mats]), arr(C.c_void_p, [o.ptr.value for o in outs]), stream()))
    torch.cuda.synchronize()
    for x, xb, ld, o, ref in zip(mats, xs, lds, outs, G.colsum_batch_ref(mats)):
        note('colsum', f'{c["name"]}-{x.shape[0]}x{x.shape[1]}', check_image(o.dev, image(o, ref), GC.BOUND['colsum']))
        single = colsum_call(lib, xb, ld, x.shape[0], x.shape[1])
        assert torch.equal(bits(o.dev), bits(single.dev)), 'colsum_batch differs from the single colsum launch of the same matrix'


def test_colsum_batch_refuses_a_fifth_sum(lib):
    x, o = flat_in(torch.ones(4)), out_buf(4)
    five = lambda t, v: (t * 5)(*[v] * 5)
    with pytest.raises(_lib.D4Error, match='d4_colsum_batch: 1 .. 4 sums'):
        _lib.check(lib.d4_colsum_batch(5, five(C.c_void_p, x.ptr.value), five(C.c_int32, 4), five(C.c_int32, 1), five(C.c_int32, 4), five(C.c_void_p, o.ptr.value),
                                       stream()))
    torch.cuda.synchronize()
    assert o.dev.isnan().all(), 'a refused call wrote an output'


# ------------------------------------------------------------------------------------------------------------------- bf16 images
@pytest.mark.parametrize('c', GC.CVT_ROWS, ids=[c['name'] for c in GC.CVT_ROWS])
def test_cvt_rows_bf16(lib, c):
    x = GC.cvt_rows_inputs(c)['x']
    src = rows_in(x, c['lds'], c['off'])
    dst = out_buf(c['rows'] * c['ldd'], dtype=torch.bfloat16)
    if c['form'] == 'vec4' or c['off']:
        aligned(True, dst.ptr, by=8)
        aligned(c['form'] == 'vec4', src.ptr)
    _lib.check(lib.d4_cvt_rows_bf16(src.ptr, c['lds'], dst.ptr, c['ldd'], c['rows'], c['cols'], stream()))
    torch.cuda.synchronize()
    check_exact(dst, image(dst, G.bf16_ref(x), c['ldd'], dtype=torch.bfloat16))


@pytest.mark.parametrize('c', GC.CVT_FLAT, ids=[c['name'] for c in GC.CVT_FLAT])
def test_cvt_f32_to_bf16(lib, c):
    x = GC.bf16_input(c['seed'], c['n'])
    src, dst = flat_in(x), out_buf(c['n'], dtype=torch.bfloat16)
    _lib.check(lib.d4_cvt_bf16(src.ptr, dst.ptr, c['n'], stream()))
    torch.cuda.synchronize()
    check_exact(dst, image(dst, G.bf16_ref(x), dtype=torch.bfloat16))


@pytest.mark.parametrize('c', GC.CVT_PAD, ids=[c['name'] for c in GC.CVT_PAD])
def test_cvt_pad_bf16(lib, c):
    x = GC.cvt_rows_inputs(c)['x']
    src = rows_in(x, c['lds'])
    dst = out_buf(c['rows'] * c['ldd'], dtype=torch.bfloat16)
    _lib.check(lib.d4_cvt_pad_bf16(src.ptr, c['lds'], dst.ptr, c['ldd'], c['rows'], c['cols'], c['cols_pad'], stream()))
    torch.cuda.synchronize()
    check_exact(dst, image(dst, G.cvt_pad_ref(x, c['cols_pad']), c['ldd'], dtype=torch.bfloat16))


@pytest.mark.parametrize('c', GC.CVT_TRANSPOSE, ids=[c['name'] for c in GC.CVT_TRANSPOSE])
def test_cvt_transpose_bf16(lib, c):
    x = GC.cvt_rows_inputs(c)['x']
    src = rows_in(x, c['lds'])
    dst = out_buf(c['cols'] * c['ldd'], dtype=torch.bfloat16)
    _lib.check(lib.d4_cvt_transpose_bf16(src.ptr, c['lds'], dst.ptr, c['ldd'], c['rows'], c['cols'], c['rows_pad'], stream()))
    torch.cuda.synchronize()
    check_exact(dst, image(dst, G.cvt_transpose_ref(x, c['rows_pad']), c['ldd'], dtype=torch.bfloat16))


def test_bf16_image_builders_refuse_what_their_stores_cannot_take(lib):
    src, dst = rows_in(torch.ones(4, 12), 13), out_buf(4 * 24 + 8, dtype=torch.bfloat16)
    off = C.c_void_p(dst.ptr.value + 2)                     # one bf16 past the 16-byte boundary
    for args, frag in (((src.ptr, 13, dst.ptr, 24, 4, 12, 12), 'cvt_pad_bf16: bad arguments'),           # cols_pad % 8 != 0
                       ((src.ptr, 13, off, 24, 4, 12, 16), 'cvt_pad_bf16: bad arguments'),                # a misaligned dst
                       ((src.ptr, 13, dst.ptr, 20, 4, 12, 16), 'cvt_pad_bf16: bad arguments')):           # ldd % 8 != 0
        with pytest.raises(_lib.D4Error, match=frag):
            _lib.check(lib.d4_cvt_pad_bf16(*args, stream()))
    with pytest.raises(_lib.D4Error, match='cvt_transpose_bf16: bad arguments'):                          # rows_pad < rows
        _lib.check(lib.d4_cvt_transpose_bf16(src.ptr, 13, dst.ptr, 8, 4, 12, 3, stream()))
    torch.cuda.synchronize()
    assert dst.dev.isnan().all(), 'a refused call wrote an output'


# ------------------------------------------------------------------------------------------------------------------- index permutations (exact)
def exact(buf, ref, ld=None):
    check_exact(buf, image(buf, ref, ld, dtype=torch.float32))


@pytest.mark.parametrize('c', GC.COPY_ROWS, ids=[c['name'] for c in GC.COPY_ROWS])
def test_copy_rows(lib, c):
    x = GC.rand(c, c['rows'], c['cols'])
    src, dst = rows_in(x, c['lds']), out_buf(c['rows'] * c['ldd'])
    _lib.check(lib.d4_copy_rows(src.ptr, c['lds'], dst.ptr, c['ldd'], c['rows'], c['cols'], stream()))
    torch.cuda.synchronize()
    exact(dst, x, c['ldd'])


@pytest.mark.parametrize('c', GC.FOLD, ids=[c['name'] for c in GC.FOLD])
def test_fold_rows(lib, c):
    W, gamma = GC.rand(c, c['rows'], c['K']), GC.rand(dict(seed=c['seed'] + 50), c['K']) if c['gamma'] else None
    Wb, gb, out = flat_in(W), (flat_in(gamma) if gamma is not None else None), out_buf(c['rows'] * c['ld'])
    _lib.check(lib.d4_fold_rows(Wb.ptr, gb.ptr if gb else None, out.ptr, c['rows'], c['K'], c['ld'], stream()))
    torch.cuda.synchronize()
    exact(out, G.fold_rows_ref(W, gamma), c['ld'])           # one correctly rounded product per element


@pytest.mark.parametrize('c', GC.SWIGLU_PACK, ids=[c['name'] for c in GC.SWIGLU_PACK])
def test_swiglu_pack_rows(lib, c):
    i, ip, k = c['inner'], c['inner_pad'], c['K']
    W, bias, gamma = GC.rand(c, 2 * i, k), GC.rand(dict(seed=c['seed'] + 50), 2 * i), GC.rand(dict(seed=c['seed'] + 60), k)
    Wp, bp = G.swiglu_pack_ref(W, bias, gamma, i, ip)
    Wb, bb, gb, Wo, bo = flat_in(W), flat_in(bias), flat_in(gamma), out_buf(2 * ip * k), out_buf(2 * ip)
    _lib.check(lib.d4_swiglu_pack_rows(Wb.ptr, bb.ptr, gb.ptr, Wo.ptr, bo.ptr, i, ip, k, stream()))
    torch.cuda.synchronize()
    exact(Wo, Wp)                                            # padding rows and their bias entries exactly zero
    exact(bo, bp)


@pytest.mark.parametrize('c', GC.BUILD_LATENT, ids=[c['name'] for c in GC.BUILD_LATENT])
def test_build_latent_input(lib, c):
    d = GC.latent_inputs(c)
    hist, ctx, x = flat_in(d['hist']), (flat_in(d['ctx']) if d['ctx'] is not None else None), flat_in(d['x'])
    out = out_buf(c['B'] * c['Tq'] * c['n_el'])
    _lib.check(lib.d4_build_latent_input(out.ptr, hist.ptr, ctx.ptr if ctx else None, x.ptr, c['B'], c['Tq'], c['n_el'], c['stride'], c['w'], stream()))
    torch.cuda.synchronize()
    if c['w'] in (0., 1.):                                   # a copy of the history / of the context noise
        exact(out, G.build_latent_ref(d['hist'], d['ctx'], d['x'], Tq=c['Tq'], w=c['w'], dtype=torch.float32))
    else:
        note('build_latent_input', c['name'], check_image(out.dev, image(out, GC.latent_expect(c, d)[0]), GC.BOUND['build_latent_input']))


@pytest.mark.parametrize('c', GC.PAD_COLS, ids=[c['name'] for c in GC.PAD_COLS])
def test_pad_cols(lib, c):
    x = GC.rand(c, c['rows'], c['cols'])
    src, dst = flat_in(x), out_buf(c['rows'] * c['cols_pad'])
    _lib.check(lib.d4_pad_cols(src.ptr, dst.ptr, c['rows'], c['cols'], c['cols_pad'], stream()))
    torch.cuda.synchronize()
    exact(dst, G.pad_cols_ref(x, c['cols_pad']))


@pytest.mark.parametrize('c', GC.VIDEO, ids=[c['name'] for c in GC.VIDEO])
def test_video_to_patches_and_back(lib, c):
    dims = (c['B'], c['C'], c['T'], c['nh'], c['nw'], c['ps'])
    v = GC.rand(c, c['B'], c['C'], c['T'], c['nh'] * c['ps'], c['nw'] * c['ps'])
    p = G.video_to_patches_ref(v, c['ps'])
    vid, pat, back = flat_in(v), out_buf(v.numel()), out_buf(v.numel())
    _lib.check(lib.d4_video_patches(vid.ptr, pat.ptr, *dims, 1, stream()))
    _lib.check(lib.d4_video_patches(pat.ptr, back.ptr, *dims, 0, stream()))         # the round trip
    p2 = GC.rand(dict(seed=c['seed'] + 70), *p.shape)                                # and the inverse on patches of its own
    pin, vout = flat_in(p2), out_buf(v.numel())
    _lib.check(lib.d4_video_patches(pin.ptr, vout.ptr, *dims, 0, stream()))
    torch.cuda.synchronize()
    exact(pat, p)
    exact(back, v)
    exact(vout, G.patches_to_video_ref(p2, *dims))


@pytest.mark.parametrize('c', GC.CACHE, ids=[c['name'] for c in GC.CACHE])
def test_cache_transfer_both_directions(lib, c):
    shape = (c['Lt'], 2, c['cache_batch'] * c['S'], c['H'], c['Tcap'], c['dh'])
    args = (c['Lt'], c['cache_batch'], c['B'], c['S'], c['H'], c['Tcap'], c['frames'])
    cache = GC.rand(c, *shape)
    ref = G.cache_to_ext_ref(cache, c['B'], c['S'], c['frames'])
    cb, ext = flat_in(cache), out_buf(ref.numel())
    _lib.check(lib.d4_cache_transfer(cb.ptr, ext.ptr, *args, 1, c['dh'], stream()))
    cache2 = out_buf(cache.numel())                                                  # an empty (NaN) cache takes the export back
    _lib.check(lib.d4_cache_transfer(cache2.ptr, ext.ptr, *args, 0, c['dh'], stream()))
    torch.cuda.synchronize()
    exact(ext, ref)
    exact(cache2, G.ext_to_cache_ref(ref, torch.full(shape, float('nan'))))          # columns past B * S and positions past `frames` untouched


@pytest.mark.parametrize('c', GC.CUNEMBED, ids=[c['name'] for c in GC.CUNEMBED])
def test_cunembed_gather_and_scatter(lib, c):
    U = GC.rand(c, c['nc'], c['mtp'], c['d'], 2)
    w = G.cunembed_gather_ref(U)
    Ub, wb, dU = flat_in(U), out_buf(w.numel()), out_buf(U.numel())
    _lib.check(lib.d4_cunembed(0, Ub.ptr, wb.ptr, c['nc'], c['mtp'], c['d'], stream()))
    _lib.check(lib.d4_cunembed(1, wb.ptr, dU.ptr, c['nc'], c['mtp'], c['d'], stream()))
    torch.cuda.synchronize()
    exact(wb, w)
    exact(dU, G.cunembed_scatter_ref(w, c['nc'], c['mtp'], c['d']))                  # heads >= 1 exactly zero


@pytest.mark.parametrize('c', GC.COORD, ids=[c['name'] for c in GC.COORD])
def test_coord_grid(lib, c):
    out = out_buf(c['nh'] * c['nw'] * c['ld'])
    _lib.check(lib.d4_coord_grid(out.ptr, c['nh'], c['nw'], c['ld'], stream()))
    torch.cuda.synchronize()
    exact(out, G.coord_grid_ref(c['nh'], c['nw'], c['ld']))


@pytest.mark.parametrize('c', GC.PACK, ids=[c['name'] for c in GC.PACK])
def test_pack_tokens(lib, c):
    Fr, P, n, nt, D = c['frames'], c['P'], c['n_lat'], c['n_total'], c['D']
    img = GC.rand(dict(seed=c['seed'] + 50), Fr, P, D)
    if c['which'] == 'decoder':
        pos, lat = GC.rand(c, P, D), GC.rand(dict(seed=c['seed'] + 60), Fr, nt, D)
        tok, comp = G.decoder_pack_ref(pos, img, lat, n)
    else:
        pos, lat = None, GC.rand(c, n, D)
        tok, comp = G.encoder_pack_ref(img, lat)
    tokens, compact = out_buf(tok.numel()), out_buf(comp.numel())
    pb, ib, lb = (flat_in(pos) if pos is not None else None), flat_in(img), flat_in(lat)
    _lib.check(lib.d4_pack_tokens(('decoder', 'encoder').index(c['which']), tokens.ptr, compact.ptr, pb.ptr if pb else None, ib.ptr, lb.ptr, Fr, P, n, nt, D, stream()))
    torch.cuda.synchronize()
    exact(tokens, tok)
    exact(compact, comp)


# ------------------------------------------------------------------------------------------------------------------- pointwise and small sums
@pytest.mark.parametrize('c', GC.SPLITK, ids=[c['name'] for c in GC.SPLITK])
def test_splitk_reduce(lib, c):
    d = GC.splitk_inputs(c)
    ldy = c['N'] + c['pad']
    part = flat_in(d['part'])
    bias = None if d['bias'] is None else flat_in(d['bias'])
    y = out_buf(c['M'] * ldy)
    _lib.check(lib.d4_splitk_reduce(part.ptr, c['S'], c['M'], c['N'], bias.ptr if bias else None, c['silu'], y.ptr, ldy, stream()))
    torch.cuda.synchronize()
    note('splitk_reduce', c['name'], check_image(y.dev, image(y, GC.splitk_expect(c, d)[0], ldy), GC.BOUND['splitk_reduce']))


@pytest.mark.parametrize('c', GC.MEAN_TOKENS, ids=[c['name'] for c in GC.MEAN_TOKENS])
def test_mean_tokens(lib, c):
    d = GC.mean_inputs(c)
    x, out = flat_in(d['x']), out_buf(c['B'] * c['d'])
    _lib.check(lib.d4_mean_tokens(x.ptr, out.ptr, c['B'], c['n'], c['d'], stream()))
    torch.cuda.synchronize()
    note('mean_tokens', c['name'], check_image(out.dev, image(out, GC.mean_expect(c, d)[0]), GC.BOUND['mean_tokens']))


@pytest.mark.parametrize('c', GC.HL_GAUSS, ids=[c['name'] for c in GC.HL_GAUSS])
def test_hl_gauss_scalar(lib, c):
    d = GC.hlg_inputs(c)
    ld, st = c['bins'] + c['pad'], c['out_stride']
    logits, centers = rows_in(d['logits'], ld), flat_in(d['centers'])
    out = out_buf((c['rows'] - 1) * st + 1)
    _lib.check(lib.d4_hl_gauss_scalar_strided(logits.ptr, ld, centers.ptr, out.ptr, st, c['rows'], c['bins'], stream()))
    torch.cuda.synchronize()
    want = torch.full((c['rows'], st), float('nan'), dtype=torch.float64)
    want[:, 0] = GC.hlg_expect(c, d)[0]
    note('hl_gauss_scalar', c['name'], check_image(out.dev, image(out, want.reshape(-1)[:out.size]), GC.BOUND['hl_gauss_scalar']))


@pytest.mark.parametrize('c', GC.EULER, ids=[c['name'] for c in GC.EULER])
def test_euler_step_rows(lib, c):
    d = GC.euler_inputs(c)
    ldx, ldp = c['n_el'] + c['padx'], c['n_el'] + c['padp']
    x, pred = rows_in(d['x'], ldx), rows_in(d['pred'], ldp)
    _lib.check(lib.d4_euler_step_rows(x.ptr, ldx, pred.ptr, ldp, c['B'], c['n_el'], c['one_minus_t'], c['dt'], stream()))
    torch.cuda.synchronize()
    note('euler_step', c['name'], check_image(x.dev, image(x, GC.euler_expect(c, d)[0], ldx), GC.BOUND['euler_step']))


@pytest.mark.parametrize('c', GC.UNARY, ids=[c['name'] for c in GC.UNARY])
def test_silu_and_tanh_rows(lib, c):
    d = GC.unary_inputs(c)
    x, y = flat_in(d['x']), out_buf(c['n'])
    _lib.check(lib.d4_unary_rows(('silu', 'tanh').index(c['op']), x.ptr, y.ptr, c['n'], stream()))
    torch.cuda.synchronize()
    note('unary', c['name'], check_image(y.dev, image(y, GC.unary_expect(c, d)[0]), GC.BOUND['unary']))


@pytest.mark.parametrize('c', GC.SILU_BWD, ids=[c['name'] for c in GC.SILU_BWD])
def test_silu_bwd(lib, c):
    d = GC.silu_bwd_inputs(c)
    dy, z, dz = flat_in(d['dy']), flat_in(d['z']), out_buf(c['n'])
    _lib.check(lib.d4_silu_bwd(dy.ptr, z.ptr, dz.ptr, c['n'], stream()))
    torch.cuda.synchronize()
    note('silu_bwd', c['name'], check_image(dz.dev, image(dz, GC.silu_bwd_expect(c, d)[0]), GC.BOUND['silu_bwd']))


@pytest.mark.parametrize('c', GC.LN_SILU_BWD, ids=[c['name'] for c in GC.LN_SILU_BWD])
def test_layernorm_silu_bwd(lib, c):
    d = GC.ln_silu_bwd_inputs(c)
    ldz, n = c['D'] + c['pad'], c['rows'] * c['D']
    z, da, g, b = rows_in(d['z'], ldz), flat_in(d['da']), flat_in(d['g']), flat_in(d['b'])
    tg, tb, dz = out_buf(n), out_buf(n), out_buf(c['rows'] * ldz)
    _lib.check(lib.d4_layernorm_silu_bwd(z.ptr, ldz, da.ptr, g.ptr, b.ptr, tg.ptr, tb.ptr, dz.ptr, c['rows'], c['D'], c['eps'], stream()))
    torch.cuda.synchronize()
    rtg, rtb, rdz = GC.ln_silu_bwd_expect(c, d)
    bound = GC.BOUND['layernorm_silu_bwd']
    note('layernorm_silu_bwd', c['name'], max(check_image(tg.dev, image(tg, rtg), bound), check_image(tb.dev, image(tb, rtb), bound),
                                               check_image(dz.dev, image(dz, rdz, ldz), bound)))


@pytest.mark.parametrize('c', GC.SWIGLU, ids=[c['name'] for c in GC.SWIGLU])
def test_swiglu_fwd_and_bwd(lib, c):
    d = GC.swiglu_inputs(c)
    rows, I, Ip = c['rows'], c['inner'], c['inner_pad']
    bwd = c['which'] == 'bwd'
    h, du = flat_in(d['h']), flat_in(d['du']) if bwd else None
    out = out_buf(rows * (2 * Ip if bwd else Ip))
    _lib.check(lib.d4_swiglu(int(bwd), h.ptr, du.ptr if bwd else None, out.ptr, rows, I, Ip, stream()))
    torch.cuda.synchronize()
    note('swiglu', c['name'], check_image(out.dev, image(out, GC.swiglu_expect(c, d)[0]), GC.BOUND['swiglu']))
    got = out.dev[GUARD:GUARD + out.size].reshape(rows, -1, Ip)[:, :, I:]
    assert bits(got).eq(0).all(), 'a pad column is not exactly +0'


# ------------------------------------------------------------------------------------------------------------------- integer inputs, copies, pad zeroing
FILL = -777                      # what an integer buffer holds wherever nothing may be written (a float one holds NaN, and prep_eval_inputs writes NaN)


def filled(n, dtype):
    return torch.full((GUARD + n + GUARD,), FILL, dtype=dtype, device=DEV)


def inner_ptr(t):
    return C.c_void_p(t.data_ptr() + GUARD * t.element_size())


def check_filled(t, want):
    """the guards still hold FILL; the inside equals `want` bit for bit (float NaN included)"""
    t, n = t.cpu(), want.numel()
    assert (t[:GUARD] == FILL).all() and (t[GUARD + n:] == FILL).all(), 'written outside the output'
    got = t[GUARD:GUARD + n]
    assert torch.equal(bits(got) if got.dtype == torch.float32 else got, bits(want.reshape(-1)) if got.dtype == torch.float32 else want.reshape(-1))


@pytest.mark.parametrize('c', GC.PREP_EVAL, ids=[c['name'] for c in GC.PREP_EVAL])
def test_prep_eval_inputs(lib, c):
    d = GC.prep_inputs(c)
    Fr, na, nc = c['B'] * c['Tq'], c['na'], c['nc']
    hist, chist = (None if t is None else t.to(DEV) for t in (d['hist'], d['chist']))
    sig, pact, pcont = filled(Fr, torch.int32), filled(Fr * na, torch.int64), filled(Fr * nc, torch.float32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _lib.check(lib.d4_prep_eval_inputs(inner_ptr(sig), inner_ptr(pact) if na else None, p(hist), c['B'], c['Tq'], na, c['frame_base'], c['hist_stride'], c['sig_val'],
                                       c['ctx_sig'], inner_ptr(pcont) if nc else None, p(chist), nc, stream()))
    torch.cuda.synchronize()
    for buf, want in zip((sig, pact, pcont), GC.prep_expect(c, d)):
        check_filled(buf, want)


@pytest.mark.parametrize('c', GC.MULTI_COPY, ids=[c['name'] for c in GC.MULTI_COPY])
def test_multi_copy(lib, c):
    segs, nd, ns = GC.multi_copy_layout(c)
    src = GC.rand(c, ns)
    sb, db = flat_in(src), out_buf(nd)
    aligned(True, sb.ptr, db.ptr)                            # so that a segment's offset alone decides between the float4 and the scalar loop
    n = len(segs)
    at = lambda buf, o: None if o is None else buf.ptr.value + 4 * o
    _lib.check(lib.d4_multi_copy(n, (C.c_void_p * n)(*[at(db, dd) for dd, _, _ in segs]), (C.c_void_p * n)(*[at(sb, so) for _, so, _ in segs]),
                                 (C.c_int64 * n)(*[k for _, _, k in segs]), stream()))
    torch.cuda.synchronize()
    exact(db, G.multi_copy_ref(segs, src, torch.full((nd,), float('nan'))))


def test_multi_copy_refuses_an_eleventh_segment(lib):
    sb, db = flat_in(torch.ones(88)), out_buf(88)
    ptrs = lambda buf: (C.c_void_p * 11)(*[buf.ptr.value + 32 * i for i in range(11)])
    with pytest.raises(_lib.D4Error, match='multi_copy: too many segments'):
        _lib.check(lib.d4_multi_copy(11, ptrs(db), ptrs(sb), (C.c_int64 * 11)(*[4] * 11), stream()))
    torch.cuda.synchronize()
    assert db.dev.isnan().all(), 'a refused call wrote an output'


@pytest.mark.parametrize('c', GC.ZERO_PAD, ids=[c['name'] for c in GC.ZERO_PAD])
def test_zero_pad_cols(lib, c):
    x = GC.rand(c, c['rows'], c['ld'])
    xb = flat_in(x)
    _lib.check(lib.d4_zero_pad_cols(xb.ptr, c['rows'], c['ld'], c['c0'], c['c1'], stream()))
    torch.cuda.synchronize()
    exact(xb, G.zero_pad_cols_ref(x, c['c0'], c['c1']))     # the zeroed columns exactly +0, every other element as it was


# ------------------------------------------------------------------------------------------------------------------- token assembly
def assemble_desc(c, d, tokens, compact):
    dev = {k: (None if v is None else v.to(DEV)) for k, v in d.items() if k != 'registers'}
    regs = flat_in(d['registers'], c['off'])
    desc = _lib.AssembleDesc()
    p = lambda t: None if t is None else t.data_ptr()
    for k in ('space', 'signal_embed', 'step_embed', 'agent_embed', 'task_embed', 'action_embed', 'action_learned', 'signal_levels', 'prev_actions', 'prev_cont',
              'cont_embed', 'tasks', 'action_offsets'):
        setattr(desc, k, p(dev[k]))
    desc.registers, desc.tokens, desc.compact = regs.ptr.value, tokens.ptr.value, compact.ptr.value if compact else None
    for k in ('B', 'Tq', 'S', 'D', 'ns', 'nr', 'na', 'nc', 'step_log2', 'signal_uniform', 'has_agent'):
        setattr(desc, k, c[k])
    return desc, (dev, regs)


@pytest.mark.parametrize('c', GC.ASSEMBLE, ids=[c['name'] for c in GC.ASSEMBLE])
def test_assemble_tokens(lib, c):
    d = GC.assemble_inputs(c)
    Fr = c['B'] * c['Tq']
    tokens = out_buf(Fr * c['S'] * c['D'])
    compact = out_buf(Fr * (c['ns'] + c['has_agent']) * c['D']) if c['compact'] else None
    desc, keep = assemble_desc(c, d, tokens, compact)
    if c['form'] == 'vec4' or c['off']:                      # the eleven tables and outputs the float4 form needs aligned, `registers` last
        aligned(c['form'] == 'vec4', *[getattr(desc, k) or 0 for k in ('tokens', 'compact', 'space', 'signal_embed', 'step_embed', 'agent_embed', 'task_embed',
                                                                     'action_embed', 'action_learned', 'cont_embed', 'registers')])
    _lib.check(lib.d4_assemble_tokens(C.byref(desc), stream()))
    torch.cuda.synchronize()
    tok, comp = G.assemble_ref(c, d)
    check_exact(tokens, image(tokens, tok, dtype=torch.float32))
    if compact:
        check_exact(compact, image(compact, comp, dtype=torch.float32))


def test_assemble_tokens_refuses_a_token_count_that_is_not_the_sum_of_its_parts(lib):
    c = GC.ASSEMBLE[0]
    d = GC.assemble_inputs(c)
    tokens = out_buf(c['B'] * c['Tq'] * (c['S'] + 1) * c['D'])
    desc, keep = assemble_desc(dict(c, S=c['S'] + 1), d, tokens, None)
    with pytest.raises(_lib.D4Error, match='d4_assemble_tokens: S 12 is not'):
        _lib.check(lib.d4_assemble_tokens(C.byref(desc), stream()))
    torch.cuda.synchronize()
    assert tokens.dev.isnan().all(), 'a refused call wrote an output'


# ------------------------------------------------------------------------------------------------------------------- clip_grad_norm_ + AdamW
@pytest.mark.parametrize('c', GC.ADAMW, ids=[c['name'] for c in GC.ADAMW])
def test_adamw_clip_three_steps(lib, c):
    family = 'adamw' if c['n'] <= 1000 else 'adamw_wide'
    d = GC.adamw_inputs(c)
    n = c['n']
    p, m, v = flat_in(d['p']), flat_in(torch.zeros(n)), flat_in(torch.zeros(n))
    scratch = out_buf(1025)
    ref = GC.adamw_expect(c, d)
    err = 0.
    for t in range(GC.ADAMW_STEPS):
        g = flat_in(d['grads'][t])
        _lib.check(lib.d4_adamw_clip(p.ptr, g.ptr, m.ptr, v.ptr, n, t + 1, c['lr'], c['b1'], c['b2'], c['eps'], c['wd'], d['max_norm'], c['grad_scale'], scratch.ptr,
                                     stream()))
        torch.cuda.synchronize()
        rp, rm, rv, rn = ref[4 * t:4 * t + 4]
        for buf, want in ((p, rp), (m, rm), (v, rv)):
            err = max(err, check_image(buf.dev, image(buf, want), GC.BOUND[family]))
        s = scratch.dev.cpu()
        assert s[:GUARD].isnan().all() and s[GUARD + 1025:].isnan().all()
        e = abs(s[GUARD].item() - rn.item()) / rn.item()
        assert e <= GC.BOUND[family], f'step {t + 1}: norm {s[GUARD].item()} against {rn.item()}: {e:.3e}'
        err = max(err, e)
    note(family, c['name'], err)


# ------------------------------------------------------------------------------------------------------------------- the whole map
def test_worst_errors_of_the_glue_families():
    for fam in GC.BOUND:
        frac, what = WORST.get(fam, (0., 'no case ran'))
        print(f'worst {fam}: {frac:.2f} of its bound ({what})')
        assert fam in WORST
