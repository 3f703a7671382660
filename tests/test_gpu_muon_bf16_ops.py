"""GPU: the Newton-Schulz operator on the bf16 matrix pipe (csrc/muon_bf16.hip) one call at a time through the C ABI,
d4_muon_plan_create_products(..., 1, ...) + d4_newton_schulz, against the float64 restatement of tests/muon_ref.py.

The ownership checks are those of tests/test_gpu_muon_ops.py: every input and output lies between NaN guards and the workspace, of exactly
d4_muon_plan_workspace_bytes, is NaN-filled: whatever a product reads, pads included, prepare / normalise must have written.
Bound: FACTOR (2) x E16 of tests/muon_bf16_cases.py, relative to the float64 output's max-abs; `lowrank` at 5 steps on its projected part."""
import ctypes as C
import math

import pytest
import torch

import muon_bf16_cases as BC
import muon_ref as R
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
MIXED = ('tiny', 'square', 'ragged', 'tall', 'odd_ld', 'lowrank', 'multi', 'two_tiles', 'three_tiles')
_REF, _ALONE = {}, {}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def reference(name, steps):
    if (name, steps) not in _REF:
        _REF[name, steps] = R.newton_schulz(BC.ns_input(name).double(), steps)
    return _REF[name, steps]


def parr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class Plan:
    """products None: d4_muon_plan_create; otherwise d4_muon_plan_create_products"""

    def __init__(self, lib, shapes, workspace_bytes=256 << 20, products=1):
        self.lib, self.h = lib, C.c_void_p(0xdead0)        # a refusal must null it
        rows = (C.c_int32 * len(shapes))(*[s[0] for s in shapes])
        cols = (C.c_int32 * len(shapes))(*[s[1] for s in shapes])
        if products is None:
            self.rc = lib.d4_muon_plan_create(len(shapes), rows, cols, workspace_bytes, C.byref(self.h))
        else:
            self.rc = lib.d4_muon_plan_create_products(len(shapes), rows, cols, workspace_bytes, products, C.byref(self.h))

    def __enter__(self):
        _lib.check(self.rc)
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.lib.d4_muon_plan_destroy(self.h)


def guarded(x):
    """x (CPU, 2-D) -> flat device buffer [NaN guard | x | NaN guard] and the pointer of x in it"""
    buf = torch.full((GUARD + x.numel() + GUARD,), math.nan)
    buf[GUARD:GUARD + x.numel()] = x.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf.data_ptr() + 4 * GUARD


def run_ns(lib, names, steps, workspace_bytes=256 << 20, inputs=None, products=1, eps=1e-7):
    """-> (outputs on the CPU, passes, workspace bytes); guards checked"""
    xs = [BC.ns_input(n) for n in names] if inputs is None else inputs
    shapes = [tuple(x.shape) for x in xs]
    ins = [guarded(x) for x in xs]
    outs = [guarded(torch.full_like(x, math.nan)) for x in xs]
    with Plan(lib, shapes, workspace_bytes, products) as plan:
        assert lib.d4_muon_plan_products(plan.h) == (products or 0)
        nbytes = lib.d4_muon_plan_workspace_bytes(plan.h)
        assert nbytes % 4 == 0
        ws = torch.full((nbytes // 4,), math.nan, device=DEV)       # NaN: whatever is read must have been written
        _lib.check(lib.d4_newton_schulz(plan.h, parr([p for _, p in ins]), parr([p for _, p in outs]), C.c_void_p(ws.data_ptr()), nbytes, steps,
                                        *R.COEFS, eps, stream()))
        passes = lib.d4_muon_plan_passes(plan.h)
    got = []
    for (buf, _), x, (ibuf, _) in zip(outs, xs, ins):
        b, i = buf.cpu(), ibuf.cpu()
        assert b[:GUARD].isnan().all() and b[GUARD + x.numel():].isnan().all(), 'a write outside the output matrix'
        assert i[:GUARD].isnan().all() and i[GUARD + x.numel():].isnan().all(), 'a write outside the input matrix'
        assert torch.equal(i[GUARD:GUARD + x.numel()], x.reshape(-1)), 'the input was modified'
        got.append(b[GUARD:GUARD + x.numel()].reshape(x.shape))
    return got, passes, nbytes


def alone(lib, name, steps):
    """the single-matrix result of a case, computed once and left unchanged"""
    if (name, steps) not in _ALONE:
        (got,), passes, _ = run_ns(lib, [name], steps)
        assert passes == 1
        _ALONE[name, steps] = got
    return _ALONE[name, steps]


def check(name, steps, got):
    assert torch.isfinite(got).all(), f'{name}: non-finite output (padding or a neighbour was read, or an element was not written)'
    err, bound = BC.ns_err(name, steps, got, reference(name, steps)), BC.FACTOR * BC.E16_NS[name, steps]
    print(f'newton_schulz bf16 {name} steps {steps}: err {err:.3e} (bound {bound:.3e}, ratio {err / bound:.2f})')
    assert err <= bound, f'{name} steps {steps}: error {err:.3e} above the bound {bound:.3e}'


@pytest.mark.parametrize('steps', BC.NS_STEPS)
@pytest.mark.parametrize('name', sorted(BC.NS_SHAPES))
def test_newton_schulz_single_matrix(lib, name, steps):
    check(name, steps, alone(lib, name, steps))


@pytest.mark.parametrize('steps', BC.NS_STEPS)
def test_newton_schulz_mixed_group_in_one_plan_and_in_passes(lib, steps):
    """every shape in ONE launch per stage (the tile table), bit for bit the single-matrix results; then with a workspace that forces >= 3 passes"""
    got, passes, _ = run_ns(lib, MIXED, steps)
    assert passes == 1
    for name, g in zip(MIXED, got):
        check(name, steps, g)
        assert torch.equal(g, alone(lib, name, steps)), f'{name}: the group changed the bits'
    # bf16 work buffers of three_tiles, the largest: 4 x (384 x 640) X images + 2 x (384 x 384) A, B, 2 bytes each
    small, passes, _ = run_ns(lib, MIXED, steps, workspace_bytes=2 * (4 * 384 * 640 + 2 * 384 * 384) + 2 * 6 * 128 * 128)
    assert passes >= 3, passes
    for name, a, b in zip(MIXED, got, small):
        assert torch.equal(a, b), f'{name}: {passes} passes changed the bits'


def test_newton_schulz_twice_bit_for_bit(lib):
    a, _, _ = run_ns(lib, MIXED, 5)
    b, _, _ = run_ns(lib, MIXED, 5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_newton_schulz_of_a_zero_matrix_is_zero(lib):
    got, _, _ = run_ns(lib, None, 5, inputs=[torch.zeros(40, 72), BC.ns_input('tall'), torch.zeros(72, 40)])
    assert float(got[0].abs().max()) == 0. and float(got[2].abs().max()) == 0.
    check('tall', 5, got[1])


def test_a_tiny_input_is_normalised_before_it_is_rounded(lib):
    """X0 = bf16(u / |u|): a power-of-two scale of the input leaves every bit of the output (the scale is formed and applied in fp32)"""
    xs = [BC.ns_input('ragged'), BC.ns_input('tall')]
    big, _, _ = run_ns(lib, None, 5, inputs=xs, eps=1e-30)
    small, _, _ = run_ns(lib, None, 5, inputs=[xs[0] * 2. ** -40, xs[1]], eps=1e-30)
    assert float(small[0].abs().max()) > 0.1
    assert torch.equal(big[0], small[0]) and torch.equal(big[1], small[1])


def test_the_result_is_the_bf16_form_s_and_the_workspace_is_not_larger(lib):
    for names in (['ragged'], ['three_tiles'], list(MIXED)):
        lo, _, lo_bytes = run_ns(lib, names, 5)
        hi, _, hi_bytes = run_ns(lib, names, 5, products=0)
        assert lo_bytes <= hi_bytes, (names, lo_bytes, hi_bytes)
        for name, a, b in zip(names, lo, hi):
            assert not torch.equal(a, b), f'{name}: the bf16 plan gave the fp32 plan\'s bits'


def test_products_0_through_the_new_entry_is_the_old_entry(lib):
    names = ['tall', 'two_tiles', 'tiny']
    new, new_passes, new_bytes = run_ns(lib, names, 5, products=0)
    old, old_passes, old_bytes = run_ns(lib, names, 5, products=None)
    assert (new_passes, new_bytes) == (old_passes, old_bytes)
    assert all(torch.equal(a, b) for a, b in zip(new, old))
    new, new_passes, new_bytes = run_ns(lib, names, 5, products=0, workspace_bytes=1310720 + 262144)
    old, old_passes, old_bytes = run_ns(lib, names, 5, products=None, workspace_bytes=1310720 + 262144)
    assert (new_passes, new_bytes) == (old_passes, old_bytes) and new_passes >= 2
    assert all(torch.equal(a, b) for a, b in zip(new, old))


@pytest.mark.parametrize('products', (2, -1))
def test_an_unknown_product_form_is_refused(lib, products):
    p = Plan(lib, [(8, 20)], products=products)
    msg = lib.d4_last_error().decode()
    assert p.rc != 0 and f'products = {products}' in msg, msg
    assert not p.h.value


def test_a_matrix_that_does_not_fit_alone_is_refused_by_name(lib):
    p = Plan(lib, [(8, 20), (150, 300)], workspace_bytes=1 << 19)
    msg = lib.d4_last_error().decode()
    assert p.rc != 0 and 'matrix 1 (150 x 300)' in msg and str(2 * (4 * 256 * 384 + 2 * 256 * 256)) in msg, msg
    assert not p.h.value


def test_the_python_entry_runs_the_same_operator(lib):
    from dreamer4_amd.optim import newton_schulz
    got, passes = newton_schulz([BC.ns_input(n).to(DEV) for n in ('ragged', 'tall')], steps=5, products='bf16')
    assert passes == 1 and all(torch.equal(g.cpu(), alone(lib, n, 5)) for g, n in zip(got, ('ragged', 'tall')))
