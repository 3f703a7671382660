"""Case tables, inputs and tolerances shared by tests/test_gpu_glue.py (the glue launchers called alone, against float64 or bit for bit) and
tests/test_glue_host.py (the same inputs on the CPU: can the bound, or the bit comparison, see a dropped row, an ignored gain, a skipped chunk,
truncation, ...?).  The scheme is attn_core_cases.py's, whose generators and FACTOR are used here.

Inputs are seeded CPU normals, shaped so that every term of a formula matters: a row 1000 times smaller than the rest (eps decides its norm),
a LayerNorm row of mean 100 and deviation 1 (a one-pass variance would lose it), gains of 1 + N(0, 1) / 2.

The tolerance.  E32[family] is the largest error of the float32 evaluation of glue_ref against its float64 evaluation over the family's cases
(max-abs relative to the output's max-abs; the worst of a case's outputs), measured on the CPU and recorded with a quarter of headroom; the GPU
bound is FACTOR x E32.  The float32 evaluation of colsum and of the AdamW norm adds its terms strictly one after the other (up to 9000 rows, a
million squares): the least accurate order, so E32 bounds every order; the kernels' trees are more accurate.  Measured (the host test prints
them): rmsnorm_rows 1.33e-7, layernorm_rows 6.72e-6 (the row of mean 100: its deviations carry the rounding of the mean), gather_space 1.53e-7,
rmsnorm_bwd 1.34e-7, colsum 3.53e-6, splitk_reduce 1.42e-7, mean_tokens 1.09e-7, hl_gauss_scalar 1.02e-7, euler_step 5.97e-8, unary 4.23e-8, build_latent_input 4.97e-8,
adamw 7.23e-7 (groups of 7 and 1000), adamw_wide 4.95e-4 (a million squares added in turn: the norm, and with an
active clip everything scaled by it; a family of its own, as the deep pool's, so that the short groups keep their tight bound), silu_bwd 6.72e-7 (at
z = +30 the factor 1 - sigmoid(z) has no correct bit left in float32 and is multiplied by z), layernorm_silu_bwd 2.68e-6, swiglu 1.53e-7 (forward and backward).
The exact families (the bf16 image builders, assemble_tokens, the index permutations and copies, prep_eval_inputs, multi_copy, zero_pad_cols, colsum_batch
against colsum) have no tolerance."""
import math

import torch

import attn_core_cases as K
import glue_ref as G

FACTOR = K.FACTOR
E32 = {'build_latent_input': 6.2e-8, 'splitk_reduce': 1.8e-7, 'mean_tokens': 1.4e-7, 'hl_gauss_scalar': 1.3e-7, 'euler_step': 7.5e-8, 'unary': 5.3e-8, 'rmsnorm_rows': 1.7e-7, 'layernorm_rows': 8.4e-6, 'gather_space': 1.9e-7, 'rmsnorm_bwd': 1.7e-7, 'colsum': 4.4e-6, 'adamw': 9.0e-7, 'adamw_wide': 6.2e-4,
       'silu_bwd': 8.4e-7, 'layernorm_silu_bwd': 3.4e-6, 'swiglu': 1.9e-7}
BOUND = {f: FACTOR * e for f, e in E32.items()}
# the kernels each choosing launcher has (the host test checks every case's `form` against the launcher's rule and that each is named)
FORMS = {'rmsnorm_rows': {'vec', 'scalar'}, 'assemble_tokens': {'vec4', 'scalar'}, 'gather_space': {'regs<1>', 'regs<2>', 'regs<4>', 'generic'},
         'cvt_rows_bf16': {'vec4', 'scalar'}, 'colsum': {'plain', 'chunked'}}
RMS_EPS, LN_EPS = 1.1920929e-07, 1e-5
GRID1D = 2048 * 256                                       # threads of grid1d (elementwise.hip); 4096 x 256: cvt_f32_to_bf16, adamw; 8192 x 256: cvt_rows_bf16


def _f32(v):
    """The float32 the C ABI hands to the kernels, as a Python float: the hyper-parameters are inputs like the tensors, and the reference takes the
    same values (1 - 0.999f is 1.3e-5 away from 0.001)."""
    return torch.tensor(v, dtype=torch.float32).item()


def _seed(table, base):
    for i, c in enumerate(table):
        c['seed'] = base + i
    return table


def _rows_input(g, rows, D, small_row=0):
    x = K._n(g, rows, D)
    x[small_row] *= 1e-3                                  # mean square 1e-6: eps (1.2e-7 / 1e-5) decides this row's norm
    return x


def _gain(g, D):
    return 1. + 0.5 * K._n(g, D)


# ------------------------------------------------------------------------------------------------------------------- rmsnorm_rows
def _rn(form, rows, D, pad=0, gamma='set'):
    """pad: extra floats of both leading dimensions; gamma 'set' / 'null' / 'off' (set, at a 4-byte offset)"""
    return dict(name=f'rms-{form}-R{rows}-D{D}-pad{pad}-g{gamma}', form=form, rows=rows, D=D, pad=pad, gamma=gamma, eps=RMS_EPS)


RMSNORM = _seed([_rn('vec', 4, 4), _rn('vec', 5, 252, pad=4), _rn('vec', 5, 4096), _rn('vec', 1, 64, gamma='null'),
                 _rn('scalar', 5, 1), _rn('scalar', 4, 6, pad=1), _rn('scalar', 1, 65), _rn('scalar', 5, 4100), _rn('scalar', 5, 64, pad=3),
                 _rn('scalar', 4, 64, gamma='off'), _rn('scalar', 5, 65, gamma='null')], 20000)


def rmsnorm_inputs(c):
    g = K._gen(c['seed'])
    return dict(x=_rows_input(g, c['rows'], c['D']), gamma=None if c['gamma'] == 'null' else _gain(g, c['D']))


def rmsnorm_expect(c, d, dtype=torch.float64, mut=()):
    return (G.rmsnorm_ref(d['x'], d['gamma'], eps=c['eps'], dtype=dtype, mut=mut),)


def rmsnorm_mutations(c):
    return ['last_row', 'last_col', 'no_eps'] + (['last_f4'] if c['form'] == 'vec' else []) + (['no_gamma'] if c['gamma'] != 'null' else [])


# ------------------------------------------------------------------------------------------------------------------- layernorm_rows
def _ln(rows, D, bias, silu, pad):
    return dict(name=f'ln-R{rows}-D{D}-b{bias}-silu{silu}-pad{pad}', rows=rows, D=D, bias=bias, silu=silu, pad=pad, eps=LN_EPS)


LAYERNORM = _seed([_ln(5, 1, 1, 0, 3), _ln(5, 63, 0, 1, 1), _ln(1, 64, 1, 1, 4), _ln(5, 65, 1, 0, 3), _ln(5, 4095, 1, 1, 1), _ln(5, 4096, 0, 0, 4),
                   _ln(1, 4096, 1, 1, 0), _ln(5, 64, 0, 0, 0)], 20100)


def layernorm_inputs(c):
    g = K._gen(c['seed'])
    x = K._n(g, c['rows'], c['D'])
    x[0] += 100.                                          # mean 100, deviation 1
    if c['rows'] > 1:
        x[-1] *= 1e-2                                     # variance 1e-4 against eps 1e-5
    return dict(x=x, g=_gain(g, c['D']), b=K._n(g, c['D']) if c['bias'] else None)


def layernorm_expect(c, d, dtype=torch.float64, mut=()):
    return (G.layernorm_ref(d['x'], d['g'], d['b'], eps=c['eps'], silu=c['silu'], dtype=dtype, mut=mut),)


def layernorm_mutations(c):
    m = ['last_row']
    if c['D'] > 1:                                        # (one column: the output is the bias alone)
        m += ['no_mean', 'last_col']
        if c['rows'] > 1:
            m.append('no_eps')
        if c['D'] <= 65:                                  # (D - 1 for D moves a wide row by 1 / 2D: below the family's bound at 4095)
            m.append('var_dm1')
    if c['bias']:
        m.append('no_bias')
    if c['silu']:
        m.append('no_silu')
    return m


# ------------------------------------------------------------------------------------------------------------------- gather_space_double_norm
def _gs(form, frames, S, first, ns, D, off=0):
    return dict(name=f'gs-{form}-F{frames}-S{S}-f{first}-ns{ns}-D{D}-off{off}', form=form, frames=frames, S=S, first=first, ns=ns, D=D, off=off, eps=RMS_EPS)


GATHER_SPACE = _seed([_gs('regs<1>', 3, 7, 1, 5, 256), _gs('regs<2>', 3, 7, 2, 3, 512), _gs('regs<4>', 2, 5, 1, 3, 1024), _gs('generic', 3, 7, 1, 5, 96),
                      _gs('generic', 3, 7, 2, 3, 512, off=1), _gs('generic', 1, 4, 3, 1, 1028)], 20200)


def gather_inputs(c):
    g = K._gen(c['seed'])
    t = K._n(g, c['frames'], c['S'], c['D'])
    t[0, c['first']] *= 1e-6                              # eps decides the first norm of this row, and its result is small enough for eps to show in the second
    return dict(tokens=t, g0=_gain(g, c['D']), g1=_gain(g, c['D']))


def gather_expect(c, d, dtype=torch.float64, mut=()):
    return (G.gather_space_ref(d['tokens'], d['g0'], d['g1'], first=c['first'], ns=c['ns'], eps=c['eps'], dtype=dtype, mut=mut),)


def gather_mutations(c):
    return ['last_row', 'last_col', 'no_gamma', 'no_eps', 'no_second', 'first_zero'] + (['last_f4'] if c['form'] != 'generic' else [])


# ------------------------------------------------------------------------------------------------------------------- rmsnorm_bwd
def _rb(rows, D, dx):
    return dict(name=f'rmsbwd-R{rows}-D{D}-dx{dx}', rows=rows, D=D, dx=dx, eps=RMS_EPS)


RMSNORM_BWD = _seed([_rb(1, 6, 1), _rb(7, 64, 1), _rb(7, 65, 0), _rb(7, 1000, 1), _rb(1, 64, 0)], 20300)


def rmsbwd_inputs(c):
    g = K._gen(c['seed'])
    return dict(x=_rows_input(g, c['rows'], c['D']), dxhat=K._n(g, c['rows'], c['D']), gamma=_gain(g, c['D']))


def rmsbwd_expect(c, d, dtype=torch.float64, mut=()):
    return G.rmsnorm_bwd_ref(d['x'], d['dxhat'], d['gamma'], eps=c['eps'], want_dx=bool(c['dx']), dtype=dtype, mut=mut)


def rmsbwd_mutations(c):
    return ['last_row', 'no_eps'] + (['no_gamma', 'no_proj'] if c['dx'] else [])


# ------------------------------------------------------------------------------------------------------------------- colsum, colsum_batch
def _cs(form, rows, cols, pad, scratch):
    """scratch: floats of scratch handed over (0: none); the chunked form needs rows >= 8192 and 16 * cols floats"""
    return dict(name=f'colsum-{form}-{rows}x{cols}-pad{pad}-s{scratch}', form=form, rows=rows, cols=cols, pad=pad, scratch=scratch)


COLSUM = _seed([_cs('plain', 1, 1, 0, 0), _cs('plain', 63, 17, 3, 0), _cs('plain', 64, 16, 0, 0), _cs('plain', 1025, 33, 1, 0), _cs('plain', 8200, 20, 0, 0),
                _cs('chunked', 8192, 20, 4, 16 * 20), _cs('chunked', 8193, 35, 1, 16 * 35), _cs('chunked', 9000, 16, 3, 16 * 16 + 5),
                _cs('plain', 8193, 35, 1, 16 * 35 - 1), _cs('plain', 8191, 20, 0, 16 * 20)], 20400)
COLSUM_BATCH = _seed([dict(name='colsum_batch-1', shapes=[(5, 3)], pad=1),
                      dict(name='colsum_batch-4', shapes=[(5, 3), (1030, 16), (64, 33), (2, 100)], pad=3)], 20500)


def colsum_inputs(c):
    return dict(x=K._n(K._gen(c['seed']), c['rows'], c['cols']))


def colsum_expect(c, d, dtype=torch.float64, mut=()):
    return (G.colsum_ref(d['x'], dtype=dtype, mut=mut),)


def colsum_mutations(c):
    return ['last_row', 'last_col'] + (['skip64'] if c['rows'] > 64 else []) + (['last_chunk'] if c['form'] == 'chunked' else [])


def colsum_batch_inputs(c):
    g = K._gen(c['seed'])
    return dict(mats=[K._n(g, r, k) for r, k in c['shapes']])


# ------------------------------------------------------------------------------------------------------------------- bf16 images
def _cv(form, rows, cols, lds, ldd, off=0):
    return dict(name=f'cvt-{form}-{rows}x{cols}-lds{lds}-ldd{ldd}-off{off}', form=form, rows=rows, cols=cols, lds=lds, ldd=ldd, off=off)


CVT_ROWS = _seed([_cv('vec4', 5, 64, 68, 72), _cv('scalar', 5, 37, 40, 40), _cv('scalar', 5, 64, 101, 72), _cv('scalar', 5, 64, 68, 72, off=1),
                  _cv('vec4', 2049, 4096, 4096, 4100),                # 8192 x 256 x 4 + 4096 elements: the float4 grid wraps
                  _cv('scalar', 517, 4057, 4057, 4058)], 20600)       # 8192 x 256 + 317 elements: the scalar grid wraps
CVT_FLAT = _seed([dict(name=f'cvt_flat-{n}', n=n) for n in (1, 255, 4096 * 256 + 257)], 20700)
_SPECIAL = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,       # +-0, +-inf, +- the largest finite float
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                                # ties: to the even mantissa below, to the even one above
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00800000, 0x80800000]        # either side of a tie; the smallest normals


def bf16_input(seed, n):
    """n float32 values as bit patterns: normal numbers with uniformly random mantissas, a quarter of them exact ties (low half 0x8000: to even, up
    and down by the bit above), and the special values at the front (as many as fit).  No NaN, no subnormal."""
    g = K._gen(seed)
    exp = torch.randint(1, 255, (n,), generator=g, dtype=torch.int64)
    man = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64)
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    tie = torch.randint(0, 4, (n,), generator=g, dtype=torch.int64) == 0
    man = torch.where(tie, (man & ~0xFFFF) | 0x8000, man)
    bits = (sign << 31) | (exp << 23) | man
    sp = torch.tensor(_SPECIAL[:n], dtype=torch.int64)
    bits[:len(sp)] = sp
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32)


def cvt_rows_inputs(c):
    return dict(x=bf16_input(c['seed'], c['rows'] * c['cols']).reshape(c['rows'], c['cols']))


def _lds_odd(cols):
    return cols // 4 * 4 + 5                               # a leading dimension that is no multiple of 4


CVT_PAD = _seed([dict(name=f'cvt_pad-{r}x{k}-pad{kp}', rows=r, cols=k, cols_pad=kp, lds=_lds_odd(k), ldd=kp + 8)
                 for r, k, kp in ((5, 1, 8), (5, 7, 8), (5, 8, 8), (5, 9, 16), (5, 100, 104), (2049, 100, 8192))], 20720)   # the last: 8192 x 256 + 1024 groups of eight
CVT_TRANSPOSE = _seed([dict(name=f'cvt_t-{r}x{k}-pad{rp}', rows=r, cols=k, rows_pad=rp, lds=k + 3, ldd=rp + 8)
                       for r, k, rp in ((1, 1, 8), (31, 33, 32), (32, 32, 32), (33, 31, 40), (100, 70, 104))], 20740)


# ------------------------------------------------------------------------------------------------------------------- index permutations (exact)
# every dimension a different small number, so that an exchanged pair of axes cannot cancel
COPY_ROWS = _seed([dict(name=f'copy-{r}x{k}', rows=r, cols=k, lds=k + 3, ldd=k + 5) for r, k in ((5, 7), (1, 1), (3, (GRID1D + 777) // 3))], 21500)
PAD_COLS = _seed([dict(name=f'pad_cols-{r}x{k}-{kp}', rows=r, cols=k, cols_pad=kp) for r, k, kp in ((5, 7, 12), (3, 8, 8), (3, 100, (GRID1D + 777) // 3))], 21520)
VIDEO = _seed([dict(name=f'video-B{B}-C{C}-T{T}-{nh}x{nw}-ps{ps}', B=B, C=C, T=T, nh=nh, nw=nw, ps=ps) for B, C, T, nh, nw, ps in ((2, 3, 5, 3, 4, 2), (1, 1, 1, 1, 1, 1),
                                                                                                                            (2, 3, 5, 7, 11, 16))], 21540)
CACHE = _seed([dict(name=f'cache-dh{dh}', Lt=2, cache_batch=4, B=2, S=3, H=5, Tcap=9, frames=7, dh=dh) for dh in (16, 32, 64)]
              + [dict(name='cache-past-grid', Lt=3, cache_batch=4, B=3, S=5, H=9, Tcap=13, frames=11, dh=64)], 21560)   # 3 x 2 x 15 x 9 x 11 x 64 = 570240 elements
CUNEMBED = _seed([dict(name=f'cunembed-nc{nc}-mtp{mtp}-d{d}', nc=nc, mtp=mtp, d=d) for nc, mtp, d in ((3, 2, 5), (1, 1, 7), (3, 2, (GRID1D + 777) // 6))], 21580)
COORD = _seed([dict(name=f'coord-{nh}x{nw}-ld{ld}', nh=nh, nw=nw, ld=ld) for nh, nw, ld in ((3, 4, 8), (1, 5, 4), (6, 1, 2), (12, 11, 3), (1, 1, 8))], 21600)
PACK = _seed([dict(name=f'pack-{w}-F{f}-P{P}-n{n}of{nt}-D{D}', which=w, frames=f, P=P, n_lat=n, n_total=nt, D=D)
              for w, f, P, n, nt, D in (('decoder', 3, 5, 2, 4, 7), ('encoder', 3, 5, 2, 2, 7), ('decoder', 3, 5, 2, 3, GRID1D // 21 + 50),
                                        ('encoder', 3, 5, 2, 2, GRID1D // 21 + 50))], 21620)


FOLD = _seed([dict(name=f'fold-{r}x{k}-g{g}', rows=r, K=k, gamma=g, ld=k + 3) for r, k, g in ((5, 7, 1), (5, 7, 0), (3, (GRID1D + 777) // 3, 1))], 21640)
SWIGLU_PACK = _seed([dict(name=f'swiglu_pack-{i}of{ip}-K{k}', inner=i, inner_pad=ip, K=k) for i, ip, k in ((5, 32, 7), (32, 32, 7), (40, 64, 7), (40, 64, 4101))], 21660)
BUILD_LATENT = _seed([dict(name=f'latent-w{w:g}-ctx{ctx}-n{n}', B=2, Tq=3, n_el=n, stride=5, w=_f32(w), ctx=ctx)
                      for w, ctx, n in ((0., 1, 7), (1., 1, 7), (0.3, 1, 7), (0.7, 1, 7), (0.3, 0, 7), (0.7, 1, (GRID1D + 777) // 6))], 21680)


def latent_inputs(c):
    g = K._gen(c['seed'])
    shape = (c['B'], c['stride'], c['n_el'])
    return dict(hist=K._n(g, *shape), ctx=K._n(g, *shape) if c['ctx'] else None, x=K._n(g, c['B'], c['n_el']))


def latent_expect(c, d, dtype=torch.float64, mut=()):
    return (G.build_latent_ref(d['hist'], d['ctx'], d['x'], Tq=c['Tq'], w=c['w'], dtype=dtype, mut=mut),)


def latent_mutations(c):
    return ['stride_as_tq', 'no_last']


def rand(c, *shape):
    return K._n(K._gen(c['seed']), *shape)


# prep_eval_inputs: the history read at a stride above Tq, from global frame 0 (the -1 / NaN sentinel in frame 0) and from a later frame; discrete,
# continuous and both kinds of action; no history at all; more frames than one block of 128 threads
def _pe(B, Tq, na, nc, base, stride, hist=1):
    return dict(name=f'prep-B{B}-Tq{Tq}-na{na}-nc{nc}-base{base}-stride{stride}-h{hist}', B=B, Tq=Tq, na=na, nc=nc, frame_base=base, hist_stride=stride, hist=hist,
                sig_val=5, ctx_sig=7)


PREP_EVAL = _seed([_pe(3, 5, 2, 0, 0, 11), _pe(3, 5, 2, 0, 4, 11), _pe(3, 5, 0, 3, 0, 11), _pe(2, 5, 2, 3, 4, 11), _pe(3, 5, 2, 3, 0, 11, hist=0), _pe(3, 1, 2, 0, 6, 11),
                   _pe(7, 19, 2, 3, 3, 23)], 21700)


def prep_inputs(c):
    g = K._gen(c['seed'])
    shape = (c['B'], c['hist_stride'])
    return dict(hist=torch.randint(0, 1000, (*shape, c['na']), generator=g) if c['hist'] and c['na'] else None,
                chist=K._n(g, *shape, c['nc']) if c['hist'] and c['nc'] else None)


def prep_expect(c, d, mut=()):
    return G.prep_eval_ref(d['hist'], d['chist'], B=c['B'], Tq=c['Tq'], na=c['na'], nc=c['nc'], frame_base=c['frame_base'], sig_val=c['sig_val'], ctx_sig=c['ctx_sig'],
                           mut=mut)


def prep_mutations(c):
    if not c['hist']:
        return []
    return ['last_row'] + (['stride_as_tq'] if c['Tq'] > 1 else []) + (['no_sentinel'] if c['frame_base'] == 0 else ['no_base'])


# multi_copy: (length, destination offset in floats past a 16-byte boundary, source offset or None for a zero fill).  Ten segments: lengths 1 / 3 / 4 / 5,
# aligned (the float4 form with its tail) and 4-byte-offset pointers on either side (the scalar form), two null sources, and one segment per form that
# is longer than the 512 x 256 threads of a segment's blocks can cover in one trip (float4: 512 x 256 x 4 floats)
MC_BIG = 512 * 256 * 4 + 777
MULTI_COPY = _seed([dict(name='multi_copy-10', segs=[(1, 0, 0), (3, 1, 0), (4, 0, 0), (5, 0, 0), (5, 0, 1), (MC_BIG, 0, 0), (4, 0, None), (5, 1, None), (3, 1, 1),
                                                     (512 * 256 + 777, 1, 3)]),
                    dict(name='multi_copy-1', segs=[(5, 0, 0)]), dict(name='multi_copy-1-off', segs=[(5, 3, 0)])], 21720)


def multi_copy_layout(c):
    """-> ([(dst offset, src offset or None, n)], floats of the destination arena, floats of the source arena): every segment starts `off` floats past a
    multiple of 4, with at least four untouched floats between two segments"""
    segs, dcur, scur = [], 0, 0
    for n, doff, soff in c['segs']:
        d = dcur + doff
        dcur = (d + n + 3) // 4 * 4 + 4
        sp = None
        if soff is not None:
            sp = scur + soff
            scur = (sp + n + 3) // 4 * 4 + 4
        segs.append((d, sp, n))
    return segs, dcur, max(scur, 4)


ZERO_PAD = _seed([dict(name=f'zero_pad-{r}x{ld}-{c0}to{c1}', rows=r, ld=ld, c0=c0, c1=c1)
                  for r, ld, c0, c1 in ((5, 13, 7, 11), (3, 8, 7, 8), (5, 9, 0, 9), (3, (4096 * 256 + 777) // 3 + 7, 2, (4096 * 256 + 777) // 3 + 3))], 21740)


# ------------------------------------------------------------------------------------------------------------------- pointwise and small sums
PAST_GRID = GRID1D + 777                                  # elements of the one case per grid1d kernel that takes a second trip of its stride loop


def _sk(S, M, N, bias, silu, pad=3):
    return dict(name=f'splitk-S{S}-{M}x{N}-b{bias}-silu{silu}', S=S, M=M, N=N, bias=bias, silu=silu, pad=pad)


SPLITK = _seed([_sk(1, 5, 7, 0, 0), _sk(3, 5, 33, 1, 1), _sk(8, 3, 17, 1, 0), _sk(3, 4, 9, 0, 1), _sk(3, 1, PAST_GRID, 1, 1)], 21000)


def splitk_inputs(c):
    g = K._gen(c['seed'])
    return dict(part=K._n(g, c['S'], c['M'], c['N']), bias=K._n(g, c['N']) if c['bias'] else None)


def splitk_expect(c, d, dtype=torch.float64, mut=()):
    return (G.splitk_reduce_ref(d['part'], d['bias'], silu=c['silu'], dtype=dtype, mut=mut),)


def splitk_mutations(c):
    return ['last_row', 'last_col'] + (['last_slice'] if c['S'] > 1 else []) + (['no_bias'] if c['bias'] else []) + (['no_silu'] if c['silu'] else [])


MEAN_TOKENS = _seed([dict(name=f'mean-B{B}-n{n}-d{d}', B=B, n=n, d=d) for B, n, d in ((3, 1, 5), (3, 7, 5), (3, 8, 5), (3, 9, 5), (3, 17, 5), (5, 3, PAST_GRID // 5))], 21100)


def mean_inputs(c):
    return dict(x=K._n(K._gen(c['seed']), c['B'], c['n'], c['d']) + 0.5)


def mean_expect(c, d, dtype=torch.float64, mut=()):
    return (G.mean_tokens_ref(d['x'], dtype=dtype, mut=mut),)


def mean_mutations(c):
    return ['last_row', 'last_col'] + (['last_token', 'sum_not_mean'] if c['n'] > 1 else [])


HL_GAUSS = _seed([dict(name=f'hlg-bins{b}', rows=5, bins=b, pad=3, out_stride=3) for b in (1, 63, 64, 65, 255)], 21200)


def hlg_inputs(c):
    g = K._gen(c['seed'])
    logits = 30. * K._n(g, c['rows'], c['bins'])                                                   # (exp overflows float32 without the max subtraction)
    logits[0, -1] = logits[0].max() + 1.                                                           # the last bin carries the first row
    return dict(logits=logits, centers=5. * K._n(g, c['bins']))


def hlg_expect(c, d, dtype=torch.float64, mut=()):
    return (G.hl_gauss_scalar_ref(d['logits'], d['centers'], dtype=dtype, mut=mut),)


def hlg_mutations(c):
    return ['last_row'] + (['last_col'] if c['bins'] > 1 else [])


EULER = _seed([dict(name=f'euler-B{B}-n{n}', B=B, n_el=n, padx=3, padp=4, one_minus_t=0.75, dt=0.25) for B, n in ((3, 37), (5, PAST_GRID // 5))], 21300)


def euler_inputs(c):
    g = K._gen(c['seed'])
    return dict(x=K._n(g, c['B'], c['n_el']), pred=K._n(g, c['B'], c['n_el']))


def euler_expect(c, d, dtype=torch.float64, mut=()):
    return (G.euler_ref(d['x'], d['pred'], one_minus_t=c['one_minus_t'], dt=c['dt'], dtype=dtype, mut=mut),)


def euler_mutations(c):
    return ['last_row', 'last_col', 'no_div']


UNARY = _seed([dict(name=f'{op}-n{n}', op=op, n=n) for op in ('silu', 'tanh') for n in (1000, PAST_GRID)], 21400)


def unary_inputs(c):
    x = (torch.rand(c['n'], generator=K._gen(c['seed'])) - 0.5) * 60.                              # +-30
    x[:2] = torch.tensor([-30., 30.])
    return dict(x=x)


def unary_expect(c, d, dtype=torch.float64, mut=()):
    return (G.unary_ref(d['x'], c['op'], dtype=dtype, mut=mut),)


def unary_mutations(c):
    return ['last_col']


# ------------------------------------------------------------------------------------------------------------------- SiLU backward, SiLU-GLU glue
SILU_BWD = _seed([dict(name=f'silu_bwd-n{n}', n=n) for n in (1000, PAST_GRID)], 21420)


def silu_bwd_inputs(c):
    g = K._gen(c['seed'])
    z = (torch.rand(c['n'], generator=g) - 0.5) * 60.                                              # +-30
    z[:2] = torch.tensor([-30., 30.])
    dy = K._n(g, c['n'])
    dy[-1] = 3.                                                                                    # (the last element is never a small one)
    z[-1] = 0.5
    return dict(dy=dy, z=z)


def silu_bwd_expect(c, d, dtype=torch.float64, mut=()):
    return (G.silu_bwd_ref(d['dy'], d['z'], dtype=dtype, mut=mut),)


def silu_bwd_mutations(c):
    return ['last_col', 'sig_only']


LN_SILU_BWD = _seed([dict(name=f'ln_silu_bwd-R{r}-D{D}-pad{pad}', rows=r, D=D, pad=pad, eps=LN_EPS) for r, D, pad in ((5, 5, 3), (1, 64, 4), (5, 64, 1), (5, 130, 3))], 21440)


def ln_silu_bwd_inputs(c):
    g = K._gen(c['seed'])
    z = K._n(g, c['rows'], c['D'])
    z[0] += 100.                                          # mean 100, deviation 1
    if c['rows'] > 1:
        z[-1] *= 1e-2                                     # variance 1e-4 against eps 1e-5
    return dict(z=z, da=K._n(g, c['rows'], c['D']), g=_gain(g, c['D']), b=K._n(g, c['D']))


def ln_silu_bwd_expect(c, d, dtype=torch.float64, mut=()):
    return G.layernorm_silu_bwd_ref(d['z'], d['da'], d['g'], d['b'], eps=c['eps'], dtype=dtype, mut=mut)


def ln_silu_bwd_mutations(c):
    return ['last_row', 'last_col', 'no_bias', 'no_silu', 'sig_only', 'no_mean_term', 'no_proj'] + (['no_eps'] if c['rows'] > 1 else [])


def _sw(which, rows, I, Ip):
    return dict(name=f'swiglu_{which}-R{rows}-{I}of{Ip}', which=which, rows=rows, inner=I, inner_pad=Ip)


SWIGLU_PAST = ((4096 * 256 + 777) // 3 + 1, ((4096 * 256 + 777) // 3 + 16) // 16 * 16)          # 3 rows of it: past the 4096 x 256 grid of grid_for
SWIGLU = _seed([_sw(w, r, i, ip) for w in ('fwd', 'bwd') for r, i, ip in ((5, 5, 16), (5, 16, 16), (3, 100, 112), (3, *SWIGLU_PAST))], 21460)


def swiglu_inputs(c):
    """h carries values in its pad columns too: the zeros there are the kernel's, not the input's"""
    g = K._gen(c['seed'])
    return dict(h=2. * K._n(g, c['rows'], 2 * c['inner_pad']), du=K._n(g, c['rows'], c['inner_pad']))


def swiglu_expect(c, d, dtype=torch.float64, mut=()):
    if c['which'] == 'fwd':
        return (G.swiglu_fwd_ref(d['h'], c['inner'], dtype=dtype, mut=mut),)
    return (G.swiglu_bwd_ref(d['h'], d['du'], c['inner'], dtype=dtype, mut=mut),)


def swiglu_mutations(c):
    return ['last_row', 'last_col', 'halves_swapped'] + (['pad_unzeroed'] if c['inner_pad'] > c['inner'] else []) + (['sig_only'] if c['which'] == 'bwd' else [])


# ------------------------------------------------------------------------------------------------------------------- assemble_tokens
ACTIONS = {'disc': (2, 0), 'cont': (0, 2), 'none': (0, 0)}          # (na, nc)
ACTION_SIZES = (3, 4)
NUM_TASKS, NUM_LEVELS, NUM_STEPS = 3, 8, 4


def _as(form, compact, has_agent, act, tasks, levels, B=2, Tq=3, D=None, off=0):
    """off: the registers table at a 4-byte offset (a scalar case by alignment alone); otherwise D = 36 makes a case scalar"""
    na, nc = ACTIONS[act]
    D = D or (36 if form == 'scalar' and not off else 40)
    ns, nr = 5, 3
    return dict(name=f'asm-{form}-c{compact}-a{has_agent}-{act}-t{tasks}-l{levels}-F{B * Tq}-D{D}-off{off}', form=form, off=off, compact=compact, has_agent=has_agent, act=act,
                tasks=tasks, levels=levels, B=B, Tq=Tq, D=D, ns=ns, nr=nr, na=na, nc=nc, S=1 + ns + nr + (1 if na or nc else 0) + has_agent, step_log2=2,
                signal_uniform=5)


# every pair of values of (form, compact, has_agent, action kind, tasks, signal levels) is in one of the first six (the host test checks); then one
# case per form past the grid of 2048 x 256 threads (91 frames of 10 tokens: 525980 float4 of a 2312-wide model, 525980 floats of a 578-wide one)
ASSEMBLE = _seed([_as('vec4', 1, 1, 'disc', 1, 1), _as('vec4', 0, 0, 'cont', 0, 0), _as('scalar', 1, 0, 'none', 1, 0), _as('scalar', 0, 1, 'disc', 0, 0, off=1),
                  _as('scalar', 1, 1, 'cont', 1, 1), _as('vec4', 0, 1, 'none', 0, 1), _as('scalar', 0, 0, 'disc', 1, 1, off=1), _as('vec4', 1, 0, 'cont', 1, 0),
                  _as('vec4', 1, 0, 'none', 0, 0), _as('vec4', 1, 1, 'none', 0, 0, B=7, Tq=13, D=2312), _as('scalar', 1, 1, 'none', 0, 0, B=7, Tq=13, D=578)],
                 20800)
ASSEMBLE_FACTORS = ('form', 'compact', 'has_agent', 'act', 'tasks', 'levels')


def assemble_inputs(c):
    g = K._gen(c['seed'])
    Fr, D, na, nc = c['B'] * c['Tq'], c['D'], c['na'], c['nc']
    ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    d = dict(space=K._n(g, Fr, c['ns'], D), signal_embed=K._n(g, NUM_LEVELS, D // 2), step_embed=K._n(g, NUM_STEPS, D // 2), registers=K._n(g, c['nr'], D),
             agent_embed=K._n(g, D), task_embed=K._n(g, NUM_TASKS, D), action_embed=K._n(g, sum(ACTION_SIZES), D), action_learned=K._n(g, D),
             cont_embed=K._n(g, 2, D), signal_levels=ri(NUM_LEVELS, Fr).to(torch.int32) if c['levels'] else None, tasks=ri(NUM_TASKS, c['B']) if c['tasks'] else None,
             action_offsets=torch.tensor([0, ACTION_SIZES[0]], dtype=torch.int32), prev_actions=None, prev_cont=None)
    if na:
        pa = torch.stack([ri(n, Fr) for n in ACTION_SIZES], 1)
        pa[:, 1] = pa[:, 1].clamp(min=1)                  # (the second type's offset shows in every frame)
        pa[2, 0] = -1                                     # one frame without a previous action
        d['prev_actions'] = pa
    if nc:
        pc = K._n(g, Fr, nc)
        pc[2, 0] = math.nan
        d['prev_cont'] = pc
    return d


def assemble_mutations(c):
    m = ['last_row']
    if c['na']:
        m += ['no_offset', 'no_sentinel']
    if c['nc']:
        m.append('no_sentinel')
    if c['compact'] and c['has_agent']:
        m.append('rank_off')
    if c['tasks'] and c['has_agent']:
        m.append('no_task')
    return m


# ------------------------------------------------------------------------------------------------------------------- d4_adamw_clip
ADAMW_STEPS = 3


def _aw(n, clip, gs, wd):
    """clip: 'off' (max_grad_norm 0), 'inactive' (twice the first step's norm), 'active' (half of it)"""
    return dict(name=f'adamw-n{n}-{clip}-gs{gs:.3g}-wd{wd:g}', n=n, clip=clip, grad_scale=_f32(gs), wd=_f32(wd), lr=_f32(0.05), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-8))


# the full cross of clip x grad_scale x weight decay over n = 7 and 1000 in turn, then two opposite corners past the grid of 4096 x 256 threads
ADAMW = _seed([_aw((7, 1000)[i % 2], clip, gs, wd) for i, (clip, gs, wd) in enumerate((c, g, w) for c in ('off', 'inactive', 'active') for g in (1., 1 / 3)
                                                                                      for w in (0., 0.01))]
              + [_aw(4096 * 256 + 1000, 'active', 1 / 3, 0.01), _aw(4096 * 256 + 1000, 'inactive', 1., 0.)], 20900)


def adamw_inputs(c):
    g = K._gen(c['seed'])
    grads = K._n(g, ADAMW_STEPS, c['n'])
    grads[1] *= 1.5                                       # the norm differs from step to step, by more than the clip's factor of two never
    norm1 = grads[0].double().norm().item() * c['grad_scale']
    return dict(p=K._n(g, c['n']), grads=grads, max_norm=_f32({'off': 0., 'inactive': 2 * norm1, 'active': norm1 / 2}[c['clip']]))


def adamw_expect(c, d, dtype=torch.float64, mut=()):
    """-> (p, m, v, norm) of step 1, of step 2, of step 3, flattened"""
    steps = G.adamw_ref(d['p'], d['grads'], lr=c['lr'], b1=c['b1'], b2=c['b2'], eps=c['eps'], wd=c['wd'], max_norm=d['max_norm'], grad_scale=c['grad_scale'],
                        dtype=dtype, mut=mut)
    return tuple(t for s in steps for t in s)


def adamw_mutations(c):
    m = ['no_bias_corr', 'tail']
    if c['wd'] > 0:
        m.append('l2_decay')
    if c['clip'] == 'inactive':
        m.append('clip_always')
    if c['grad_scale'] != 1.:
        m.append('scale_not_in_norm')
    return m


ALL_TABLES = dict(rmsnorm_rows=RMSNORM, layernorm_rows=LAYERNORM, gather_space=GATHER_SPACE, rmsnorm_bwd=RMSNORM_BWD, colsum=COLSUM, colsum_batch=COLSUM_BATCH,
                  cvt_rows_bf16=CVT_ROWS, cvt_f32_to_bf16=CVT_FLAT, cvt_pad_bf16=CVT_PAD, cvt_transpose_bf16=CVT_TRANSPOSE, assemble_tokens=ASSEMBLE, adamw=ADAMW,
                  copy_rows=COPY_ROWS, fold_rows=FOLD, swiglu_pack_rows=SWIGLU_PACK, build_latent_input=BUILD_LATENT, pad_cols=PAD_COLS, video_patches=VIDEO, cache_transfer=CACHE, cunembed=CUNEMBED, coord_grid=COORD, pack_tokens=PACK,
                  splitk_reduce=SPLITK, mean_tokens=MEAN_TOKENS, hl_gauss_scalar=HL_GAUSS, euler_step=EULER, unary=UNARY, prep_eval_inputs=PREP_EVAL,
                  multi_copy=MULTI_COPY, zero_pad_cols=ZERO_PAD, silu_bwd=SILU_BWD, layernorm_silu_bwd=LN_SILU_BWD, swiglu=SWIGLU)
NUMERIC = dict(rmsnorm_rows=(RMSNORM, rmsnorm_inputs, rmsnorm_expect, rmsnorm_mutations), layernorm_rows=(LAYERNORM, layernorm_inputs, layernorm_expect, layernorm_mutations),
               gather_space=(GATHER_SPACE, gather_inputs, gather_expect, gather_mutations), rmsnorm_bwd=(RMSNORM_BWD, rmsbwd_inputs, rmsbwd_expect, rmsbwd_mutations),
               colsum=(COLSUM, colsum_inputs, colsum_expect, colsum_mutations), adamw=([c for c in ADAMW if c['n'] <= 1000], adamw_inputs, adamw_expect, adamw_mutations),
               adamw_wide=([c for c in ADAMW if c['n'] > 1000], adamw_inputs, adamw_expect, adamw_mutations),
               splitk_reduce=(SPLITK, splitk_inputs, splitk_expect, splitk_mutations), mean_tokens=(MEAN_TOKENS, mean_inputs, mean_expect, mean_mutations),
               hl_gauss_scalar=(HL_GAUSS, hlg_inputs, hlg_expect, hlg_mutations), euler_step=(EULER, euler_inputs, euler_expect, euler_mutations),
               unary=(UNARY, unary_inputs, unary_expect, unary_mutations), silu_bwd=(SILU_BWD, silu_bwd_inputs, silu_bwd_expect, silu_bwd_mutations),
               layernorm_silu_bwd=(LN_SILU_BWD, ln_silu_bwd_inputs, ln_silu_bwd_expect, ln_silu_bwd_mutations),
               swiglu=(SWIGLU, swiglu_inputs, swiglu_expect, swiglu_mutations),
               build_latent_input=([c for c in BUILD_LATENT if c['w'] not in (0., 1.)], latent_inputs, latent_expect, latent_mutations))
