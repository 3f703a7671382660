"""Case tables, inputs, tolerances and fixture loading shared by tests/test_gpu_tok_reg_ops.py (the two operators of csrc/tok_reg.hip called alone through
their C entry points), tests/test_gpu_tok_reg.py (the mirror against the reference fixture tok_reg.npz) and tests/test_tok_reg_host.py (the same tables
and fixture on the CPU).  The scheme is tests/tok_train_cases.py's.

SIGReg cases (K, N, d, M; knots on a domain): one row (closed form); ragged rows; more than one block of 64 rows (the reduction across workgroups);
d no multiple of 4 and fewer slices than a wave; 1024 slices; d at its limit of 128; 2 knots; 16 knots (none at zero); 4 knots on (0, 3) (no symmetry to
use); rows scaled by 20 (angles of hundreds of radians); 2048 standard-normal rows (the loss near its floor: C - phi cancels).
Orthogonality cases (F, n, d): n = 1 (exact zero); 2 x 2; the fixture's 6 x 6 x 8; a full wave of rows; one past; n >> d; d at its limit; orthonormal
rows plus 1e-3 noise; a frame of identical rows.

Two notes on the last two.  Orthonormal rows: their own Gram is the identity to 1e-3 (the uncentred sum of squared off-diagonal entries is ~1e-6, which is
what an identity through the d x d Gram would lose), but the operator centres over the rows first, and n centred rows are never nearly orthogonal (unit
rows that sum to zero with positive weights have sum_{i != j} G_ij^2 >= n / (n - 1)), so the operator's loss on this input is of order one: the case
probes the input, not a loss of 1e-6.  Identical rows: the entries are multiples of 1/8 and n = 8, so the column mean is exact in every summation order,
the centred rows are exactly zero, and loss and gradient are exactly zero, here as in the reference (with generic values the mean of n equal
numbers is rounded, in torch as anywhere, and the normalisation blows that rounding up to unit vectors).

The tolerance.  E32[family] is the largest error of the float32 evaluation of tok_reg_ref against its float64 evaluation over the family's cases (max-abs
relative to the output's max-abs, `rel_err`), measured on the CPU (the host test prints them) and recorded with a quarter of headroom; the GPU bound is
FACTOR (8) x E32.  The float32 evaluation adds the long sums in the kernels' own order (blocks of 64 rows, then the blocks; a frame's rows per wave, then
the waves), so E32 is the rounding the kernels' arithmetic must show, not that of a worse order.  The families separate what has a different
conditioning, so that a hard case does not loosen the bound of the ordinary ones.  SIGReg (the worse of loss and gradient): `sigreg`,
`sigreg_large_angle` (the angle t p itself carries a rounding of 1e-5 rad at 300 rad), `sigreg_floor` (the loss is a difference of nearly equal numbers).
Orthogonality: `ortho_loss` (the loss of every case), `ortho_grad` (the gradient of the random frames), `ortho_grad_near_orthonormal` (the gradient of the
orthonormal-rows case, 4.5e-3 left of terms of order one).
Measured: sigreg 1.01e-6 (the gradient with 2 knots), sigreg_large_angle 1.83e-6, sigreg_floor 1.96e-6, ortho_loss 6.72e-8, ortho_grad 1.70e-6 (the
256-row frame), ortho_grad_near_orthonormal 1.57e-5.
The 2 x 2 x 4 case has no relative measure for its gradient: two centred rows are opposite whatever x is, the loss is the constant 2 and the true
gradient exactly 0.  It is held to an absolute bound instead, `two_rows_grad_bound`: an entry of the computed gradient is what is left of two terms
G_ij y_j / norm_i and y_i (y_i . dy_i) / norm_i of magnitude at most (4 / F) / norm_i each, each carrying a few roundings of relative size 2^-24 (the
mean, the centring, the normalisation, the dot product), so what is left is within FACTOR x 2^-24 x (4 / F) / min_i norm_i."""
import torch

import attn_core_cases as K
import tok_train_cases as TC

FACTOR = K.FACTOR
E32 = {'sigreg': 1.27e-6, 'sigreg_large_angle': 2.29e-6, 'sigreg_floor': 2.45e-6, 'ortho_loss': 8.4e-8, 'ortho_grad': 2.12e-6, 'ortho_grad_near_orthonormal': 1.96e-5}
BOUND = {f: FACTOR * e for f, e in E32.items()}
ROWS_PER_BLOCK, MAX_DIM, MAX_KNOTS, MAX_SLICES, ORTHO_MAX_ROWS = 64, 128, 64, 4096, 1024           # csrc/kernels.h: SIGREG_*, ORTHO_*
DEFAULT = dict(lo=-5., hi=5., knots=17)                                                             # sigreg's defaults


def _sig(name, K_, N, d, M, seed, family='sigreg', scale=1.5, shift=0.3, **kn):
    return dict(name=name, K=K_, N=N, d=d, M=M, seed=seed, family=family, scale=scale, shift=shift, **{**DEFAULT, **kn})


SIGREG_CASES = [
    _sig('one_row', 1, 1, 4, 1, 7500),
    _sig('ragged', 2, 77, 8, 64, 7501),
    _sig('row_blocks', 2, 300, 32, 256, 7502),
    _sig('odd_dim', 1, 40, 6, 5, 7503),
    _sig('slices_1024', 1, 16, 64, 1024, 7504),
    _sig('dim_128', 1, 16, 128, 64, 7505),
    _sig('knots_2', 2, 77, 8, 64, 7506, knots=2),
    _sig('knots_16', 2, 77, 8, 64, 7507, knots=16),
    _sig('asymmetric', 2, 77, 8, 64, 7508, lo=0., hi=3., knots=4),
    _sig('scaled_20', 2, 77, 8, 64, 7509, family='sigreg_large_angle', scale=20., shift=0.),
    _sig('floor', 1, 2048, 8, 16, 7510, family='sigreg_floor', scale=1., shift=0.),
]
ORTHO_CASES = [dict(name=f'{kind}_{F}x{n}x{d}', F=F, n=n, d=d, kind=kind, seed=7600 + i, family='ortho_loss',
                    grad_family='ortho_grad_near_orthonormal' if kind == 'orthonormal' else 'ortho_grad') for i, (F, n, d, kind) in enumerate(
    [(3, 1, 8, 'randn'), (2, 2, 4, 'randn'), (6, 6, 8, 'randn'), (2, 64, 16, 'randn'), (1, 65, 32, 'randn'), (1, 256, 8, 'randn'), (1, 130, 128, 'randn'),
     (2, 4, 16, 'orthonormal'), (1, 8, 16, 'identical')])]
EXACT_ZERO = ('randn_3x1x8', 'identical_1x8x16')
ZERO_GRADIENT = 'randn_2x2x4'                             # loss 2, true gradient exactly 0: two_rows_grad_bound
REFUSED_SIGREG = [dict(K=1, N=4, d=129, M=8, knots=17), dict(K=1, N=4, d=8, M=8, knots=1), dict(K=1, N=4, d=8, M=4097, knots=17)]
REFUSED_ORTHO = [dict(F=1, n=4, d=129), dict(F=1, n=1025, d=8)]


def sigreg_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    x = torch.randn(c['K'], c['N'], c['d'], generator=g) * c['scale'] + c['shift']
    return dict(x=x, projs=torch.randn(c['M'], c['d'], generator=g))


def ortho_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    F, n, d = c['F'], c['n'], c['d']
    if c['kind'] == 'orthonormal':
        q = torch.linalg.qr(torch.randn(F, d, n, generator=g, dtype=torch.float64)).Q.transpose(-1, -2)      # F n d, orthonormal rows
        return dict(x=(q + 1e-3 * torch.randn(F, n, d, generator=g, dtype=torch.float64)).float())
    if c['kind'] == 'identical':
        return dict(x=(torch.randint(-8, 9, (F, 1, d), generator=g).float() / 8).expand(F, n, d).contiguous())
    return dict(x=torch.randn(F, n, d, generator=g) + 0.5)


def sigreg_part_floats(K_, N, M, knots):
    """d4_sigreg_part_floats: the partial sums of the characteristic function per block of rows, plus the loss partials of the second pass"""
    return K_ * -(-N // ROWS_PER_BLOCK) * M * knots * 2 + -(-K_ * M * knots // 256)


rel_err = TC.rel_err


def two_rows_grad_bound(x):
    """the absolute bound on the gradient of a frame of two rows, whose true value is 0 (module docstring)"""
    xd = x.double()
    norms = (xd - xd.mean(dim=-2, keepdim=True)).norm(dim=-1)
    return FACTOR * 2. ** -24 * (4. / x[..., 0, 0].numel()) / norms.min().item()


# ----------------------------------------------------------------------------- the fixture of the whole training forward
REG_CASES = ('reg', 'reg2', 'reg_nonorm')
TERMS = ('recon', 'latent_ortho', 'latent_consistency', 'latent_sigreg')
NORMALIZER_KEYS = {f: f'{f}_loss_normalizer.exp_avg_sq' for f in TERMS}
LOSS_TOL, VALUE_TOL, GRAD_TOL, STATE_TOL = TC.LOSS_TOL, TC.VALUE_TOL, TC.GRAD_TOL, TC.STATE_TOL


def fixture():
    """(constructor kwargs with the three weights, weights by state_dict key, recorded cases): the narrow tokenizer of tok_train.npz (the generator asserts
    the weights equal) with the regularisers on"""
    kw, W, _ = TC.fixture()
    g = TC.load_parts('tok_reg.npz')
    w = float(g['cfg_weight'])
    reg = dict(latent_sigreg_loss_weight=w, latent_ortho_loss_weight=w, latent_consistency_loss_weight=w,
               latent_sigreg_loss_kwargs=dict(num_slices=int(g['cfg_num_slices'])))
    return kw, reg, W, g


def case_draws(g, name):
    return dict(TC.case_draws(g, name), sigreg_projs=torch.from_numpy(g[f'{name}_sigreg_projs']))


def norm_states(g, name, when, dtype=torch.float32):
    return {f: torch.from_numpy(g[f'{name}_norm_{when}/{f}']).to(dtype) for f in TERMS}
