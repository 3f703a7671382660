"""CPU: the host side of MuonAdamAtan2 (dreamer4_amd/optim.py): the restated arithmetic is sane, the parameter partition, the
`muon_parameters()` names against the reference's (tests/golden/muon_names.json), state_dict round trip, refusals, the bound symbols."""
import pytest
import torch

import muon_cases as MC
import muon_ref as R
from dreamer4_amd import DynamicsWorldModel, MuonAdamAtan2, VideoTokenizer, _lib
from dreamer4_amd.build import build


def test_restated_newton_schulz_orthogonalises_a_full_rank_input():
    # aspect ratio 3 or more: the normalised input's singular values then lie within a factor ~4 of each other (Marchenko-Pastur edges
    # 1 -+ sqrt(rows / cols)), all inside the basin the five iterations lift into the band.  A square Gaussian's smallest singular value is O(1 / n)
    # of the largest and is not lifted in five iterations whatever the coefficients; that is conditioning, not what this checks.
    for shape in ((32, 96), (96, 32), (64, 256)):
        u = torch.randn(shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        sv = torch.linalg.svdvals(R.newton_schulz(u, 5))
        assert 0.3 <= float(sv.min()) and float(sv.max()) <= 1.25, (shape, float(sv.min()), float(sv.max()))


def test_restated_update_scales():
    assert R.update_scale('spectral', 340, 64) == pytest.approx((340 / 64) ** 0.5) and R.update_scale('spectral', 64, 340) == 1.
    assert R.update_scale('match_rms_adam', 64, 340) == pytest.approx(0.2 * 340 ** 0.5) and R.update_scale('none', 9, 2) == 1.


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 6)), torch.nn.Parameter(torch.zeros(6)), torch.nn.Parameter(torch.zeros(3, 3))]


def test_partition_removes_muon_parameters_by_identity():
    w, b, other = _params()
    twin = torch.nn.Parameter(torch.zeros(4, 6))            # equal to w in value and shape, another tensor
    opt = MuonAdamAtan2([w], [w, b, other, twin])
    muon, adam = opt.param_groups
    assert muon['use_muon'] and not adam['use_muon']
    assert [id(p) for p in muon['params']] == [id(w)]
    assert [id(p) for p in adam['params']] == [id(b), id(other), id(twin)]


def test_a_tensor_in_both_lists_is_refused_when_not_removed():
    w, b, other = _params()
    with pytest.raises(ValueError, match='both'):
        MuonAdamAtan2([w], [w, b], remove_muon_params_from_params=False)
    MuonAdamAtan2([w], [b, other], remove_muon_params_from_params=False)


def test_muon_takes_2d_tensors_only():
    w, b, other = _params()
    with pytest.raises(ValueError, match='2-D'):
        MuonAdamAtan2([w, b], [other])


def test_bad_update_scale_raises():
    w, b, other = _params()
    with pytest.raises(ValueError, match='muon_update_scale'):
        MuonAdamAtan2([w], [b], muon_update_scale='rms')


@pytest.mark.parametrize('key,cls', [('dynamics', DynamicsWorldModel), ('tokenizer', VideoTokenizer)])
def test_muon_parameters_are_the_reference_s(key, cls):
    fx = MC.fixture()[key]
    m = cls(**fx['kwargs'])
    names = {id(p): k for k, p in m.named_parameters()}
    muon = m.muon_parameters()
    assert len({id(p) for p in muon}) == len(muon)
    assert sorted(names[id(p)] for p in muon) == fx['names']
    assert all(p.ndim == 2 for p in muon)
    if key == 'dynamics':           # depth 4, a time block every 2 layers: time layers and every pool are in
        assert 'transformer.layers.1.2.fn.to_v.weight' in fx['names'] and 'transformer.final_special_ff.fn.proj_out.weight' in fx['names']
        assert not any(k.startswith(('latents_to_spatial_tokens', 'to_latent_pred')) for k in fx['names'])


def test_state_dict_round_trip():
    w, b, other = _params()
    opt = MuonAdamAtan2([w], [w, b, other], lr=3e-4, muon_lr=2e-3, weight_decay=0.1, muon_nesterov=False, muon_update_scale='match_rms_adam')
    opt.state[w] = dict(step=4, exp_avg=torch.full_like(w, 0.5))
    opt.state[b] = dict(step=3, exp_avg=torch.full_like(b, 0.25), exp_avg_sq=torch.full_like(b, 2.))
    sd = opt.state_dict()
    w2, b2, other2 = _params()
    new = MuonAdamAtan2([w2], [w2, b2, other2])
    new.load_state_dict(sd)
    assert new.state[w2]['step'] == 4 and torch.equal(new.state[w2]['exp_avg'], opt.state[w]['exp_avg'])
    assert new.state[b2]['step'] == 3 and torch.equal(new.state[b2]['exp_avg_sq'], opt.state[b]['exp_avg_sq'])
    assert other2 not in new.state
    muon, adam = new.param_groups
    assert muon['use_muon'] and muon['muon_lr'] == 2e-3 and not muon['muon_nesterov'] and muon['muon_update_scale'] == 'match_rms_adam'
    assert adam['lr'] == 3e-4 and adam['weight_decay'] == 0.1


def test_a_cpu_model_is_refused_at_step():
    w, b, other = _params()
    opt = MuonAdamAtan2([w], [b, other])
    for p in (w, b):
        p.grad = torch.ones_like(p)
    with pytest.raises(_lib.D4Error, match='no CPU fallback'):
        opt.step()
    assert float(w.detach().abs().max()) == 0. and not opt.state       # nothing moved


def test_the_header_s_muon_symbols_are_bound():
    build()
    lib = _lib.load()
    for name in ('d4_muon_plan_create', 'd4_muon_plan_destroy', 'd4_muon_plan_workspace_bytes', 'd4_muon_plan_passes', 'd4_muon_step', 'd4_newton_schulz',
                 'd4_multi_table_bytes', 'd4_sumsq_multi', 'd4_adam_atan2_multi'):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
