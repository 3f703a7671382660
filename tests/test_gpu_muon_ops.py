"""GPU: the operators of csrc/muon.hip one call at a time through the C ABI against the float64 restatement of tests/muon_ref.py:
d4_newton_schulz (the Muon step's own launchers) on groups that hit every index path, d4_adam_atan2_multi, d4_sumsq_multi, and the refusals.

Every input and output of the Newton-Schulz cases lies between NaN guards: a read past a matrix poisons the output, a write past it clears a
guard.  Bound: FACTOR (8) x E32 of tests/muon_cases.py, relative to the float64 output's max-abs."""
import ctypes as C
import math

import pytest
import torch

import muon_cases as MC
import muon_ref as R
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
MIXED = ('tiny', 'square', 'ragged', 'tall', 'odd_ld', 'multi', 'two_tiles')
_REF = {}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def reference(name, steps):
    if (name, steps) not in _REF:
        _REF[name, steps] = R.newton_schulz(MC.ns_input(name).double(), steps)
    return _REF[name, steps]


def parr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class Plan:
    def __init__(self, lib, shapes, workspace_bytes=256 << 20):
        self.lib, self.h = lib, C.c_void_p()
        rows = (C.c_int32 * len(shapes))(*[s[0] for s in shapes])
        cols = (C.c_int32 * len(shapes))(*[s[1] for s in shapes])
        self.rc = lib.d4_muon_plan_create(len(shapes), rows, cols, workspace_bytes, C.byref(self.h))

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


def run_ns(lib, names, steps, workspace_bytes=256 << 20, inputs=None):
    """-> (outputs on the CPU, passes); guards checked"""
    xs = [MC.ns_input(n) for n in names] if inputs is None else inputs
    shapes = [tuple(x.shape) for x in xs]
    ins = [guarded(x) for x in xs]
    outs = [guarded(torch.full_like(x, math.nan)) for x in xs]
    with Plan(lib, shapes, workspace_bytes) as plan:
        ws = torch.full((lib.d4_muon_plan_workspace_bytes(plan.h) // 4,), math.nan, device=DEV)       # NaN: whatever is read must have been written
        _lib.check(lib.d4_newton_schulz(plan.h, parr([p for _, p in ins]), parr([p for _, p in outs]), C.c_void_p(ws.data_ptr()), ws.numel() * 4, steps,
                                        *R.COEFS, 1e-7, stream()))
        passes = lib.d4_muon_plan_passes(plan.h)
    got = []
    for (buf, _), x, (ibuf, _) in zip(outs, xs, ins):
        b, i = buf.cpu(), ibuf.cpu()
        assert b[:GUARD].isnan().all() and b[GUARD + x.numel():].isnan().all(), 'a write outside the output matrix'
        assert torch.equal(i[GUARD:GUARD + x.numel()], x.reshape(-1)), 'the input was modified'
        got.append(b[GUARD:GUARD + x.numel()].reshape(x.shape))
    return got, passes


def check(name, steps, got):
    assert not got.isnan().any(), f'{name}: NaN in the output (padding or a neighbour was read, or an element was not written)'
    err, bound = MC.rel_err(got, reference(name, steps)), MC.FACTOR * MC.E32_NS[name, steps]
    print(f'newton_schulz {name} steps {steps}: err {err:.3e} (bound {bound:.3e})')
    assert err <= bound, f'{name} steps {steps}: error {err:.3e} above the bound {bound:.3e}'


@pytest.mark.parametrize('steps', MC.NS_STEPS)
@pytest.mark.parametrize('name', sorted(MC.NS_SHAPES))
def test_newton_schulz_single_matrix(lib, name, steps):
    (got,), passes = run_ns(lib, [name], steps)
    assert passes == 1
    check(name, steps, got)


@pytest.mark.parametrize('steps', MC.NS_STEPS)
def test_newton_schulz_mixed_group_in_one_plan_and_in_passes(lib, steps):
    """every shape in ONE launch per stage (the tile table), bit for bit the single-matrix results; then with a workspace that forces >= 3 passes"""
    got, passes = run_ns(lib, MIXED, steps)
    assert passes == 1
    for name, g in zip(MIXED, got):
        check(name, steps, g)
        (alone,), _ = run_ns(lib, [name], steps)
        assert torch.equal(g, alone), f'{name}: the group changed the bits'
    # work buffers: 4 x 128 x 128 floats for the one-tile shapes, up to 2 x 256 x 384 + 2 x 256 x 256 for two_tiles (1.25 MiB)
    small, passes = run_ns(lib, MIXED, steps, workspace_bytes=1310720 + 262144)
    assert passes >= 3, passes
    for name, a, b in zip(MIXED, got, small):
        assert torch.equal(a, b), f'{name}: {passes} passes changed the bits'


def test_newton_schulz_twice_bit_for_bit(lib):
    a, _ = run_ns(lib, MIXED, 5)
    b, _ = run_ns(lib, MIXED, 5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_newton_schulz_of_a_zero_matrix_is_zero(lib):
    got, _ = run_ns(lib, None, 5, inputs=[torch.zeros(40, 72), MC.ns_input('tall'), torch.zeros(72, 40)])
    assert float(got[0].abs().max()) == 0. and float(got[2].abs().max()) == 0.
    check('tall', 5, got[1])


def test_the_python_entry_runs_the_same_operator(lib):
    from dreamer4_amd.optim import newton_schulz
    got, passes = newton_schulz([MC.ns_input(n).to(DEV) for n in ('ragged', 'tall')], steps=5)
    ref, _ = run_ns(lib, ['ragged', 'tall'], 5)
    assert passes == 1 and all(torch.equal(g.cpu(), r) for g, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------ multi-tensor kernels
def table_for(lib, sizes):
    numel = (C.c_int64 * len(sizes))(*sizes)
    nbytes = lib.d4_multi_table_bytes(len(sizes), numel)
    assert nbytes > 0
    return numel, torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize('steps', (1, 3))
def test_adam_atan2_multi(lib, steps):
    W, grads = MC.adam_inputs()
    hp = MC.ADAM_HP
    W = [w.to(DEV) for w in W]
    M, V = [torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in W]
    numel, table = table_for(lib, MC.ADAM_SIZES)
    held = None
    for t in range(steps):
        G = [g.to(DEV) for g in grads[t]]
        ptrs = [parr([x.data_ptr() for x in xs]) for xs in (W, G, M, V)]
        now = tuple(g.data_ptr() for g in G)
        _lib.check(lib.d4_adam_atan2_multi(len(W), numel, *ptrs, C.c_void_p(table.data_ptr()), table.numel(), int(now != held), t + 1, hp['lr'], *hp['betas'],
                                           hp['weight_decay'], hp['a'], hp['b'], None, 0., stream()))
        torch.cuda.synchronize()
        held = now
    ref = MC.adam_reference(torch.float64, steps)
    bound = MC.FACTOR * MC.E32_ADAM[steps]
    for what, got, want in zip(('param', 'exp_avg', 'exp_avg_sq'), (W, M, V), ref):
        for n, g, w in zip(MC.ADAM_SIZES, got, want):
            err = MC.rel_err(g.cpu(), w)
            print(f'adam_atan2 {what} n={n} steps {steps}: err {err:.3e} (bound {bound:.3e})')
            assert err <= bound, (what, n, err, bound)


def test_adam_atan2_multi_applies_the_clip(lib):
    W, grads = MC.adam_inputs()
    hp = MC.ADAM_HP
    G = [g.to(DEV) for g in grads[0]]
    norm_sq = torch.tensor([sum(float((g.double() ** 2).sum()) for g in grads[0])], dtype=torch.float32, device=DEV)
    coef = R.clip_coef(grads[0], 0.5)
    assert coef < 1.
    Wd = [w.to(DEV) for w in W]
    M, V = [torch.zeros_like(w) for w in Wd], [torch.zeros_like(w) for w in Wd]
    numel, table = table_for(lib, MC.ADAM_SIZES)
    ptrs = [parr([x.data_ptr() for x in xs]) for xs in (Wd, G, M, V)]
    _lib.check(lib.d4_adam_atan2_multi(len(W), numel, *ptrs, C.c_void_p(table.data_ptr()), table.numel(), 1, 1, hp['lr'], *hp['betas'], hp['weight_decay'],
                                       hp['a'], hp['b'], C.c_void_p(norm_sq.data_ptr()), 0.5, stream()))
    for w, g, got_m, got_g in zip(W, grads[0], M, G):
        _, m, _ = R.adam_atan2_step(w.double(), g.double() * coef, torch.zeros_like(w).double(), torch.zeros_like(w).double(), 1, **hp)
        assert MC.rel_err(got_m.cpu(), m) <= MC.FACTOR * MC.E32_ADAM[1]
        assert torch.equal(got_g.cpu(), g), 'the gradient itself must stay untouched'


def test_sumsq_multi(lib):
    xs = MC.sumsq_inputs()
    X = [x.to(DEV) for x in xs]
    numel, table = table_for(lib, [x.numel() for x in xs])
    out = torch.full((2, 1), math.nan, device=DEV)
    for k in range(2):
        _lib.check(lib.d4_sumsq_multi(len(X), numel, parr([x.data_ptr() for x in X]), C.c_void_p(table.data_ptr()), table.numel(), int(k == 0),
                                      C.c_void_p(out[k].data_ptr()), stream()))
    want = sum(float((x.double() ** 2).sum()) for x in xs)
    got = out.cpu()
    err = abs(float(got[0]) - want) / want
    print(f'sumsq_multi: err {err:.3e} (bound {MC.FACTOR * MC.E32_SUMSQ:.3e})')
    assert err <= MC.FACTOR * MC.E32_SUMSQ
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), 'two runs differ'


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('shapes,frag', [([(4, 0)], 'cols = 0'), ([(8, 8), (0, 3)], 'matrix 1 has rows = 0'), ([(-1, 5)], 'rows = -1')])
def test_plan_refuses_empty_matrices(lib, shapes, frag):
    p = Plan(lib, shapes)
    assert p.rc != 0 and frag in lib.d4_last_error().decode(), lib.d4_last_error()
    assert not p.h.value


def test_plan_names_the_matrix_that_exceeds_the_budget(lib):
    p = Plan(lib, [(8, 20), (150, 300)], workspace_bytes=1 << 20)
    msg = lib.d4_last_error().decode()
    assert p.rc != 0 and 'matrix 1 (150 x 300)' in msg and str(4 * (2 * 256 * 384 + 2 * 256 * 256)) in msg, msg


def test_null_pointers_are_refused_before_any_launch(lib):
    x = MC.ns_input('tiny').to(DEV)
    out = torch.full_like(x, math.nan)
    with Plan(lib, [(8, 20)]) as plan:
        ws = torch.empty(lib.d4_muon_plan_workspace_bytes(plan.h), dtype=torch.uint8, device=DEV)
        rc = lib.d4_newton_schulz(plan.h, parr([None]), parr([out.data_ptr()]), C.c_void_p(ws.data_ptr()), ws.numel(), 5, *R.COEFS, 1e-7, stream())
        assert rc != 0 and 'pointer 0 is null' in lib.d4_last_error().decode()
        rc = lib.d4_newton_schulz(plan.h, parr([x.data_ptr()]), parr([out.data_ptr()]), C.c_void_p(ws.data_ptr()), 16, 5, *R.COEFS, 1e-7, stream())
        assert rc != 0 and 'workspace' in lib.d4_last_error().decode()
    torch.cuda.synchronize()
    assert out.isnan().all()
    numel, table = table_for(lib, [4, 4])
    g = torch.ones(4, device=DEV)
    rc = lib.d4_sumsq_multi(2, numel, parr([g.data_ptr(), None]), C.c_void_p(table.data_ptr()), table.numel(), 1, C.c_void_p(g.data_ptr()), stream())
    assert rc != 0 and 'grads[1] is null' in lib.d4_last_error().decode()
    ptrs = [parr([g.data_ptr(), g.data_ptr()]) for _ in range(3)] + [parr([g.data_ptr(), None])]
    rc = lib.d4_adam_atan2_multi(2, numel, *ptrs, C.c_void_p(table.data_ptr()), table.numel(), 1, 1, 1e-3, 0.9, 0.99, 0., 1.27, 1., None, 0., stream())
    assert rc != 0 and '[1] is null' in lib.d4_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), torch.ones(4))
