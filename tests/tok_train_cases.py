"""Case tables, inputs, tolerances and fixture loading shared by tests/test_gpu_tok_train_ops.py (the pixel-side operators of the tokenizer's training
forward called alone through the C entry points), tests/test_gpu_tok_train.py (the mirror against the reference fixtures) and
tests/test_tok_train_host.py (the same tables and fixtures on the CPU).  The scheme is tests/glue_cases.py's.

Shapes: the smallest at which each kernel can go wrong.  Patch geometry ps 4 / C 3 (a patch row of 48 floats) and ps 2 / C 1 (a row of 4: one float4);
patch grids 4 x 6 and 1 x 1; 1 and 3 frames; two clips with different times, one of them t = 0.  LayerNorm backward and mask rows: dim 32 (lanes 8 .. 63
of a wave idle) and 96; 1 row, 144 rows (18 row tiles of 8: more than one block) and 77 rows (no multiple of the tile, nor of the 4
waves: a ragged last tile), one case with padded input rows; masks with no, every and some rows set.

The tolerance.  E32[family] is the largest error of the float32 evaluation of tok_train_ref against its float64 evaluation over the family's cases
(max-abs relative to the output's max-abs; the worst of a case's outputs), measured on the CPU (the host test prints them) and recorded with a quarter
of headroom; the GPU bound is FACTOR (8) x E32.  The float32 evaluation adds the terms of a column sum and of the loss sum strictly one after the
other: the least accurate order, so E32 bounds every order, the kernels' partials-then-reduction among them.  Measured: flow_noised_patches 4.12e-8,
layernorm_rows_bwd 4.79e-6 (the row of mean 100: its deviations carry the rounding of the mean), mask_rows_bwd 2.68e-7, recon_loss 1.59e-6 (the loss: up to
6912 squares added in turn).  mask_rows_fwd is a copy: exact."""
import glob
import itertools
import os

import numpy as np
import torch

import attn_core_cases as K

FACTOR = K.FACTOR
E32 = {'flow_noised_patches': 5.2e-8, 'layernorm_rows_bwd': 6.0e-6, 'mask_rows_bwd': 3.4e-7, 'recon_loss': 2.0e-6}
BOUND = {f: FACTOR * e for f, e in E32.items()}
LN_EPS = 1e-5
ROW_TILE, MAX_DIM, LOSS_PARTS = 8, 1024, 1024              # csrc/kernels.h: TOK_ROW_TILE, 256 * TOK_NJ, TOK_LOSS_PARTS

GEOMS = [dict(ps=ps, C=C, nh=nh, nw=nw, T=T, B=2, times=(0., 0.5))
         for (ps, C), (nh, nw), T in itertools.product(((4, 3), (2, 1)), ((4, 6), (1, 1)), (1, 3))]
FLOW_CASES = [dict(g, name=f"ps{g['ps']}c{g['C']}_{g['nh']}x{g['nw']}_T{g['T']}", seed=7100 + i) for i, g in enumerate(GEOMS)]
LOSS_CASES = [dict(g, v_space=v, name=f"{'v' if v else 'x'}_ps{g['ps']}c{g['C']}_{g['nh']}x{g['nw']}_T{g['T']}", seed=7200 + 2 * i + v)
              for i, g in enumerate(GEOMS) for v in (1, 0)]
LN_CASES = [dict(rows=r, D=D, pad=0, name=f'r{r}_d{D}', seed=7300 + i) for i, (r, D) in enumerate(itertools.product((1, 144, 77), (32, 96)))]
LN_CASES.append(dict(rows=77, D=96, pad=8, name='r77_d96_pad8', seed=7310))
MASK_CASES = [dict(rows=r, D=D, kind=k, name=f'{k}_r{r}_d{D}', seed=7400 + i)
              for i, ((r, D), k) in enumerate(itertools.product(((144, 32), (77, 96), (1, 32)), ('none', 'all', 'mixed')))]
REFUSED_GEOMS = [dict(ps=1, C=3, nh=2, nw=2, T=1, B=1), dict(ps=1, C=1, nh=4, nw=4, T=2, B=1)]       # patch rows of 3 and 1 floats


def part_floats(rows, D):
    """d4_tok_rows_part_floats: one row of D partial sums per block of ROW_TILE rows."""
    return -(-rows // ROW_TILE) * D


def geom_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    shape = (c['B'], c['C'], c['T'], c['nh'] * c['ps'], c['nw'] * c['ps'])
    video, noise = torch.rand(shape, generator=g), torch.randn(shape, generator=g)
    rows = torch.randn(c['B'], c['T'], c['nh'], c['nw'], c['ps'] * c['ps'] * c['C'], generator=g)
    return dict(video=video, noise=noise, times=torch.tensor(c['times']), recon_rows=rows)


def ln_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    x = torch.randn(c['rows'], c['D'], generator=g)
    x[0] = 100. + torch.randn(c['D'], generator=g)                   # mean 100, deviation 1: a one-pass variance would lose it
    if c['rows'] > 2:
        x[2] *= 1e-3                                                   # eps decides this row's scale
    return dict(x=x, dy=torch.randn(c['rows'], c['D'], generator=g), g=1. + torch.randn(c['D'], generator=g) / 2)


def mask_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    rows, D = c['rows'], c['D']
    mask = {'none': torch.zeros(rows, dtype=torch.bool), 'all': torch.ones(rows, dtype=torch.bool), 'mixed': torch.rand(rows, generator=g) < 0.4}[c['kind']]
    if c['kind'] == 'mixed':
        mask[0], mask[rows - 1] = (rows > 1), True
    return dict(x=torch.randn(rows, D, generator=g), dy=torch.randn(rows, D, generator=g), token=torch.randn(D, generator=g), mask=mask)


def rel_err(a, b):
    """max |a - b| relative to max |b| (b: the float64 reference)"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30)).item()


# ----------------------------------------------------------------------------- fixtures of the whole training forward
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
UNREAD = 'decoder.transformer.final_special_'                                       # the decoder never reads its last latent token back
UNUSED = 'final_special_cross_attn.fn.to_learned_value_residual_mix.'             # constructed, never called with residual values (dreamer4.py:3227-3234)
NARROW_CASES = ('train', 'train2', 'nonorm', 'xspace', 'image')
LOSS_TOL, VALUE_TOL, GRAD_TOL, STATE_TOL = 1e-5, 2e-4, 1e-3, 1e-4                 # tests/test_gpu_backward.py's, on train.npz


def load_parts(name):
    """A fixture written in parts of under 1 MiB (tools/gen_tok_train_golden.py): NAME.npz, NAME.p1.npz, ... merged into one dict."""
    stem = name[:-4]
    out = {}
    for path in [os.path.join(GOLDEN, name)] + sorted(glob.glob(os.path.join(GOLDEN, stem + '.p*.npz'))):
        z = np.load(path, allow_pickle=False)
        out.update({k: z[k] for k in z.files})
    return out


def fixture(wide=False):
    """(constructor kwargs, weights by state_dict key, recorded cases) of a reference tokenizer fixture."""
    suffix = '_wide' if wide else ''
    w = load_parts(f'weights_tok_train{suffix}.npz')
    kw = {k[4:]: v.tolist() for k, v in w.items() if k.startswith('cfg_')}
    W = {k: torch.from_numpy(v) for k, v in w.items() if not k.startswith(('cfg_', 'meta_'))}
    return kw, W, load_parts(f'tok_train{suffix}.npz')


def case_draws(g, name):
    t = lambda k: torch.from_numpy(g[f'{name}_{k}'])
    return dict(patch_mask=t('patch_mask'), time_indices=t('time_indices'), noise=t('noise'))


def case_grads(g, name):
    pre = f'{name}_grad/'
    return {k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}


def time_attention(key, kw):
    """key names a parameter of a time layer's attention block (layers.N.2.fn.*, N a time layer)"""
    if '.layers.' not in key or '.2.fn.' not in key:
        return False
    return (int(key.split('.layers.')[1].split('.')[0]) + 1) % kw['time_block_every'] == 0


def has_gradient(key, kw=None, frames=None):
    """Every parameter of the tokenizer but the two groups nothing reads — and, on one-frame input, but the time layers' attention blocks: the belief
    projection cancels an attention over a single key, the block's output is identically zero and its gradients are rounding noise around zero
    (NOISE_FLOOR of the case's largest gradient, as tools/gen_tok_train_golden.py asserts of the reference's)."""
    if frames == 1 and time_attention(key, kw):
        return False
    return not key.startswith(UNREAD) and UNUSED not in key


NOISE_FLOOR = 1e-6
