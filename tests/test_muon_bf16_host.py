"""CPU: the host side of MuonAdamAtan2's bf16 products: the emulated contract (tests/muon_bf16_ref.py) is the restated iteration once
its roundings are taken out, the recorded E16 table is complete and honest, the emulation still orthogonalises, and the Python surface."""
import pytest
import torch

import muon_bf16_cases as BC
import muon_bf16_ref as E
import muon_cases as MC
import muon_ref as R
from dreamer4_amd import MuonAdamAtan2, _lib
from dreamer4_amd.build import build
from dreamer4_amd.optim import PRODUCTS, newton_schulz


@pytest.mark.parametrize('chunk', (None, 32))
def test_without_the_roundings_the_emulation_is_the_restated_iteration(chunk):
    for name in ('tiny', 'tall', 'odd_ld', 'three_tiles'):
        u = BC.ns_input(name).double()
        for steps in BC.NS_STEPS:
            err = MC.rel_err(E.newton_schulz(u, steps, round=False, chunk=chunk), R.newton_schulz(u, steps))
            assert err <= 1e-12, (name, steps, err)


def test_the_roundings_are_there():
    u = BC.ns_input('ragged')
    X = E.newton_schulz(u.double(), 1)
    assert torch.equal(X, X.to(torch.bfloat16).double()) and not torch.equal(X, E.newton_schulz(u.double(), 1, round=False))


def test_the_recorded_table_is_complete_and_not_below_a_fresh_measurement():
    assert set(BC.E16_NS) == {(n, s) for n in BC.NS_SHAPES for s in BC.NS_STEPS}
    assert set(BC.NS_SHAPES) == set(MC.NS_SHAPES) | {'three_tiles'} and BC.NS_SHAPES['three_tiles'] == (260, 520)
    assert set(BC.E16_TRAJECTORY) == set(MC.TRAJECTORY)
    for key in (('tiny', 5), ('lowrank', 5), ('ragged', 1)):
        fresh = BC.measure_ns(*key)
        assert 0. < fresh <= BC.E16_NS[key], (key, fresh, BC.E16_NS[key])


def test_the_emulation_orthogonalises_gaussians():
    # the band of tests/test_muon_host.py: five iterations lift every singular value of a well-conditioned input into it, bf16 roundings included
    for shape in ((512, 1365), (256, 1024)):
        u = torch.randn(shape, generator=torch.Generator().manual_seed(3))
        sv = torch.linalg.svdvals(E.newton_schulz(u, 5, chunk=32).double())
        print(shape, float(sv.min()), float(sv.max()))
        assert 0.3 <= float(sv.min()) and float(sv.max()) <= 1.25, (shape, float(sv.min()), float(sv.max()))


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 6)), torch.nn.Parameter(torch.zeros(6)), torch.nn.Parameter(torch.zeros(3, 3))]


def test_an_unknown_product_form_raises_at_construction():
    w, b, other = _params()
    with pytest.raises(ValueError, match='muon_products'):
        MuonAdamAtan2([w], [b, other], muon_products='fp8')
    with pytest.raises(ValueError, match='products'):
        newton_schulz([torch.zeros(4, 6)], products='fp8')


def test_the_mode_is_an_attribute_and_not_in_the_state_dict():
    w, b, other = _params()
    lo = MuonAdamAtan2([w], [w, b, other], muon_products='bf16')
    hi = MuonAdamAtan2([w], [w, b, other], muon_products='fp32')
    assert lo.muon_products == 'bf16' and hi.muon_products == 'fp32' and MuonAdamAtan2([w], [b]).muon_products == 'fp32'
    for opt in (lo, hi):
        opt.state[w] = dict(step=2, exp_avg=torch.full_like(w, 0.5))
    a, b_ = lo.state_dict(), hi.state_dict()
    assert a.keys() == b_.keys() and [g.keys() for g in a['param_groups']] == [g.keys() for g in b_['param_groups']]
    assert not any('muon_products' in g for g in a['param_groups'])
    assert {k: v.keys() for k, v in a['state'].items()} == {k: v.keys() for k, v in b_['state'].items()}
    hi.load_state_dict(a)                                   # written under 'bf16', loaded under 'fp32'
    assert hi.muon_products == 'fp32' and hi.state[w]['step'] == 2


def test_the_new_symbols_are_bound():
    build()
    lib = _lib.load()
    for name in ('d4_muon_plan_create_products', 'd4_muon_plan_products'):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.d4_version() == 2 and PRODUCTS == {'fp32': 0, 'bf16': 1}       # the plan's `products` values of include/d4hip.h
