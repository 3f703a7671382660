"""GPU: the two operators of csrc/tok_reg.hip, each called alone through its C entry point (d4_sigreg_fwd_bwd, d4_latent_ortho_fwd_bwd) on the cases
of tests/tok_reg_cases.py.

A case asserts
  * the values: loss and d loss / d x against the float64 restatement (tests/tok_reg_ref.py) within BOUND[family] = 8 x E32[family], the error
    relative to the output's max-abs; the two frames whose loss is exactly zero give exactly zero and a zero gradient; the frame of two rows, whose
    true gradient is exactly zero, is held to the absolute bound tok_reg_cases.two_rows_grad_bound;
  * untouched memory: loss, gradient and scratch sit between NaN guards that are still NaN afterwards, and the scratch is exactly the size the query
    entry returns;
  * determinism: a second call into fresh buffers gives the same bits (every sum has a fixed order: no float atomics).
Sizes outside the limits are refused with the library's error.  The autograd functions scale the saved gradient by the upstream gradient on both
routes; the patch permutation of an un-patchified tensor of patch rows gives the rows back bit for bit (what lets the consistency pass feed the
decoder's rows to the encoder).

    family                        measured E32   recorded E32   bound (8 x)
    sigreg                        1.01e-6        1.27e-6        1.0e-5
    sigreg_large_angle            1.83e-6        2.29e-6        1.8e-5
    sigreg_floor                  1.96e-6        2.45e-6        2.0e-5
    ortho_loss                    6.72e-8        8.4e-8         6.7e-7
    ortho_grad                    1.70e-6        2.12e-6        1.7e-5
    ortho_grad_near_orthonormal   1.57e-5        1.96e-5        1.6e-4"""
import ctypes as C
import math

import pytest
import torch

import tok_reg_cases as RC
import tok_reg_ref as R
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
ids = lambda table: [c['name'] for c in table]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n floats of device memory between two runs of GUARD NaNs, all NaN before the call"""
    def __init__(self, n):
        self.n, self.buf = n, torch.full((n + 2 * GUARD,), math.nan, device='cuda')

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def value(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert host[:GUARD].isnan().all() and host[GUARD + self.n:].isnan().all(), 'a write outside the output'
        return host[GUARD:GUARD + self.n]


def run_sigreg(lib, c, d):
    x, projs = d['x'].cuda(), d['projs'].cuda()
    n = lib.d4_sigreg_part_floats(c['K'], c['N'], c['M'], c['knots'])
    assert n == RC.sigreg_part_floats(c['K'], c['N'], c['M'], c['knots'])
    loss, dx, part = Guarded(1), Guarded(x.numel()), Guarded(n)
    _lib.check(lib.d4_sigreg_fwd_bwd(_lib.ptr(x), _lib.ptr(projs), c['K'], c['N'], c['d'], c['M'], c['lo'], c['hi'], c['knots'], loss.ptr, dx.ptr, part.ptr, n,
                                     stream()))
    part.value()
    return loss.value(), dx.value().reshape(x.shape)


def run_ortho(lib, c, d):
    x = d['x'].cuda()
    n = lib.d4_latent_ortho_part_floats(c['F'])
    loss, dx, part = Guarded(1), Guarded(x.numel()), Guarded(n)
    _lib.check(lib.d4_latent_ortho_fwd_bwd(_lib.ptr(x), c['F'], c['n'], c['d'], loss.ptr, dx.ptr, part.ptr, n, stream()))
    part.value()
    return loss.value(), dx.value().reshape(x.shape)


@pytest.mark.parametrize('c', RC.SIGREG_CASES, ids=ids(RC.SIGREG_CASES))
def test_sigreg_against_float64(lib, c):
    d = RC.sigreg_inputs(c)
    loss, dx = run_sigreg(lib, c, d)
    want_loss, want_dx = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'])
    e_loss, e_dx = RC.rel_err(loss, want_loss.reshape(1)), RC.rel_err(dx, want_dx)
    print(f"sigreg {c['name']}: loss {loss.item():.6e} (float64 {want_loss.item():.6e}) err {e_loss:.3e}, dx err {e_dx:.3e}, bound {RC.BOUND[c['family']]:.3e}")
    assert e_loss <= RC.BOUND[c['family']] and e_dx <= RC.BOUND[c['family']], (e_loss, e_dx)
    again = run_sigreg(lib, c, d)
    assert torch.equal(again[0], loss) and torch.equal(again[1], dx), 'two calls on the same input give the same bits'


@pytest.mark.parametrize('c', RC.ORTHO_CASES, ids=ids(RC.ORTHO_CASES))
def test_latent_ortho_against_float64(lib, c):
    d = RC.ortho_inputs(c)
    loss, dx = run_ortho(lib, c, d)
    if c['name'] in RC.EXACT_ZERO:
        assert loss.item() == 0. and torch.isfinite(dx).all() and not dx.any(), 'exactly zero, and a zero gradient'
    else:
        want_loss, want_dx = R.latent_ortho_ref(d['x'])
        e_loss = RC.rel_err(loss, want_loss.reshape(1))
        if c['name'] == RC.ZERO_GRADIENT:
            e_dx, bound_dx = dx.abs().max().item(), RC.two_rows_grad_bound(d['x'])
        else:
            e_dx, bound_dx = RC.rel_err(dx, want_dx), RC.BOUND[c['grad_family']]
        print(f"ortho {c['name']}: loss {loss.item():.6e} (float64 {want_loss.item():.6e}) err {e_loss:.3e} (bound {RC.BOUND[c['family']]:.3e}), "
              f"dx err {e_dx:.3e} (bound {bound_dx:.3e})")
        assert e_loss <= RC.BOUND[c['family']] and e_dx <= bound_dx, (e_loss, e_dx)
    again = run_ortho(lib, c, d)
    assert torch.equal(again[0], loss) and torch.equal(again[1], dx), 'two calls on the same input give the same bits'


def test_sizes_outside_the_limits_are_refused(lib):
    buf = torch.zeros(1 << 16, device='cuda')
    p = _lib.ptr(buf)
    for c in RC.REFUSED_SIGREG:
        assert lib.d4_sigreg_fwd_bwd(p, p, c['K'], c['N'], c['d'], c['M'], -5., 5., c['knots'], p, p, p, 1 << 30, stream()) != 0, c
        assert lib.d4_last_error()
    for c in RC.REFUSED_ORTHO:
        assert lib.d4_latent_ortho_fwd_bwd(p, c['F'], c['n'], c['d'], p, p, p, 1 << 30, stream()) != 0, c
    assert lib.d4_sigreg_fwd_bwd(p, p, 1, 4, 8, 8, -5., 5., 17, p, p, p, 3, stream()) != 0, 'a scratch below the query is refused'
    assert lib.d4_sigreg_fwd_bwd(p, None, 1, 4, 8, 8, -5., 5., 17, p, p, p, 1 << 30, stream()) != 0, 'null argument'
    assert lib.d4_latent_ortho_fwd_bwd(p, 2, 4, 8, p, p, p, 1, stream()) != 0, 'a scratch below the query is refused'
    torch.cuda.synchronize()
    assert not buf.any(), 'a refused call writes nothing'
    from dreamer4_amd import trunk_ops
    with pytest.raises(_lib.D4Error):
        trunk_ops.sigreg(torch.zeros(1, 4, 129, device='cuda'), torch.ones(8, 129, device='cuda'))
    with pytest.raises(_lib.D4Error):
        trunk_ops.latent_ortho(torch.zeros(1, 1025, 8, device='cuda'))


@pytest.mark.parametrize('route', ['0', '1'])
def test_autograd_functions_scale_by_the_upstream_gradient(lib, route, monkeypatch):
    from dreamer4_amd import trunk_ops
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', route)
    c = RC.SIGREG_CASES[1]
    d = RC.sigreg_inputs(c)
    x = d['x'].cuda().reshape(c['K'], 7, 11, c['d']).requires_grad_()                  # (k, ..., d): the middle axes are the samples
    loss = trunk_ops.sigreg(x, d['projs'].cuda(), (c['lo'], c['hi']), c['knots'])
    (loss * 3.5).backward()
    want_loss, want_dx = run_sigreg(lib, c, d)
    assert torch.equal(loss.detach().cpu().reshape(1), want_loss) and torch.equal(x.grad.cpu().reshape(want_dx.shape), want_dx * 3.5)
    c = RC.ORTHO_CASES[2]
    d = RC.ortho_inputs(c)
    x = d['x'].cuda().reshape(2, 3, c['n'], c['d']).requires_grad_()
    loss = trunk_ops.latent_ortho(x)
    (loss * -0.25).backward()
    want_loss, want_dx = run_ortho(lib, c, d)
    assert torch.equal(loss.detach().cpu().reshape(1), want_loss) and torch.equal(x.grad.cpu().reshape(want_dx.shape), want_dx * -0.25)


def test_patch_permutation_of_unpatchified_rows_is_the_identity():
    from dreamer4_amd import ops, trunk_ops
    for (B, T, nh, nw, ps, Cc) in ((2, 3, 4, 6, 4, 3), (1, 1, 1, 1, 2, 1), (2, 2, 3, 5, 2, 3)):
        rows = torch.randn(B, T, nh, nw, ps * ps * Cc, generator=torch.Generator().manual_seed(B + T + nh)).cuda()
        assert torch.equal(trunk_ops.video_to_patches(ops.patches_to_video_impl(rows, Cc, ps), ps), rows)
