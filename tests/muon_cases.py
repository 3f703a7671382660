"""Shapes, inputs and tolerances of the MuonAdamAtan2 tests (tests/test_muon_host.py, test_gpu_muon_ops.py, test_gpu_muon.py).

The tolerance is the scheme of DESIGN.md 17.  E32[case] is the largest error of the float32 CPU evaluation of tests/muon_ref.py against its float64
evaluation, as max-abs difference relative to the float64 output's max-abs, measured by `python tests/muon_cases.py` and recorded below with 25 %
headroom; the GPU bound is FACTOR x E32."""
import json
import os

import torch

import muon_ref as R

FACTOR = 8.
HERE = os.path.dirname(os.path.abspath(__file__))

# ------------------------------------------------------------------------------------------------ Newton-Schulz operator
# name -> (rows, cols); 'lowrank' inputs are rank-4 plus 1e-3 noise
NS_SHAPES = {
    'tiny': (8, 20),              # less than one tile
    'square': (64, 64),           # square, exact MFMA-tile multiple
    'ragged': (40, 72),           # rows and cols both ragged
    'tall': (72, 40),             # needs the transpose
    'odd_ld': (40, 173),          # leading dimension not a multiple of 4 (like inner = 1365)
    'lowrank': (40, 173),         # the same shape on a low-rank-plus-noise input
    'multi': (96, 341),           # several MFMA tiles with a ragged edge
    'two_tiles': (150, 300),      # more than one 128-tile per side: off-diagonal (mirrored) tiles of the symmetric stages
}
NS_STEPS = (1, 5)


def ns_input(name):
    r, c = NS_SHAPES[name]
    g = torch.Generator().manual_seed(1000 + sorted(NS_SHAPES).index(name))
    if name == 'lowrank':
        return (torch.randn(r, 4, generator=g) @ torch.randn(4, c, generator=g) + 1e-3 * torch.randn(r, c, generator=g)).float()
    return torch.randn(r, c, generator=g)


def rel_err(got, ref):
    """max-abs difference relative to the reference's max-abs"""
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# measured by `python tests/muon_cases.py` (float32 CPU against float64), x 1.25
E32_NS = {
    ('tiny', 1): 1.90e-07, ('tiny', 5): 1.14e-06,
    ('square', 1): 1.04e-07, ('square', 5): 2.23e-06,
    ('ragged', 1): 9.90e-08, ('ragged', 5): 1.92e-06,
    ('tall', 1): 1.61e-07, ('tall', 5): 2.02e-06,
    ('odd_ld', 1): 1.05e-07, ('odd_ld', 5): 3.79e-06,
    ('lowrank', 1): 2.01e-07, ('lowrank', 5): 3.99e-05,
    ('multi', 1): 4.74e-07, ('multi', 5): 3.65e-06,
    ('two_tiles', 1): 2.27e-07, ('two_tiles', 5): 4.59e-06,
}

# ------------------------------------------------------------------------------------------------ multi-tensor Adam-atan2 / squared norm
ADAM_SIZES = (1, 7, 1024, 5000)
ADAM_HP = dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1, a=1.27, b=1.)
E32_ADAM = {1: 8.81e-08, 3: 1.93e-07}          # steps -> E32 over parameters, exp_avg and exp_avg_sq
E32_SUMSQ = 7.42e-06                           # squares added term after term, the least accurate order: bounds every order


def adam_inputs():
    g = torch.Generator().manual_seed(77)
    W = [torch.randn(n, generator=g) for n in ADAM_SIZES]
    grads = [[torch.randn(n, generator=g) * 10. ** float(torch.randint(-3, 2, (1,), generator=g)) for n in ADAM_SIZES] for _ in range(3)]
    return W, grads


def adam_reference(dtype, steps):
    W, grads = adam_inputs()
    W = [w.to(dtype) for w in W]
    M, V = [torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in W]
    for t in range(steps):
        for i in range(len(W)):
            W[i], M[i], V[i] = R.adam_atan2_step(W[i], grads[t][i].to(dtype), M[i], V[i], t + 1, **ADAM_HP)
    return W, M, V


def sumsq_inputs():
    g = torch.Generator().manual_seed(78)
    return [torch.randn(n, generator=g) for n in (1, 7, 4096, 4097, 50000)]


# ------------------------------------------------------------------------------------------------ the optimiser on the fixture's small model
def fixture():
    with open(os.path.join(HERE, 'golden', 'muon_names.json')) as f:
        return json.load(f)


TRAJECTORY = {
    'nesterov_spectral_clip': dict(lr=1e-2, weight_decay=0.1, muon_nesterov=True, muon_update_scale='spectral', max_grad_norm=0.5),
    'plain_rms': dict(lr=1e-2, muon_lr=2e-2, weight_decay=0.1, muon_nesterov=False, muon_update_scale='match_rms_adam'),
}
TRAJECTORY_STEPS = 3
SKIPPED = 'transformer.layers.1.3.fn.proj_in.weight'        # the parameter whose .grad stays None
UNLISTED = ('register_tokens', 'transformer.layers.0.2.fn.to_q.weight')     # given to neither list
E32_TRAJECTORY = {'nesterov_spectral_clip': 3.56e-07, 'plain_rms': 1.03e-06}


def small_dynamics():
    from dreamer4_amd import DynamicsWorldModel
    torch.manual_seed(0)
    return DynamicsWorldModel(**fixture()['dynamics']['kwargs'])


def trajectory_gradients(model):
    """three steps of synthetic gradients per parameter, O(1) entries (norm far above 0.5: the clip is active)"""
    g = torch.Generator().manual_seed(11)
    out = []
    for _ in range(TRAJECTORY_STEPS):
        out.append({k: (None if k == SKIPPED or p.numel() == 0 else torch.randn(p.shape, generator=g)) for k, p in model.named_parameters()})
    return out


def trajectory_reference(model, case, dtype):
    names = {id(p): k for k, p in model.named_parameters()}
    muon = {names[id(p)] for p in model.muon_parameters()}
    params = {k: p for k, p in model.named_parameters() if k not in UNLISTED and p.numel() > 0}
    grads = [{k: g for k, g in step.items() if k in params} for step in trajectory_gradients(model)]
    return R.optimiser_trajectory(params, muon, grads, dtype, **TRAJECTORY[case])


def measure():
    """every E32 of this file, unrounded"""
    out = {'ns': {}, 'adam': {}, 'trajectory': {}}
    for name in NS_SHAPES:
        for steps in NS_STEPS:
            u = ns_input(name)
            out['ns'][(name, steps)] = rel_err(R.newton_schulz(u, steps), R.newton_schulz(u.double(), steps))
    for steps in (1, 3):
        lo, hi = adam_reference(torch.float32, steps), adam_reference(torch.float64, steps)
        out['adam'][steps] = max(rel_err(a, b) for A, B in zip(lo, hi) for a, b in zip(A, B))
    xs = sumsq_inputs()
    import numpy as np
    acc = np.float32(0.)
    for x in xs:                                  # term after term: the least accurate order
        for sq in (x * x).numpy():
            acc = np.float32(acc + sq)
    out['sumsq'] = abs(float(acc) - sum(float((x.double() ** 2).sum()) for x in xs)) / sum(float((x.double() ** 2).sum()) for x in xs)
    m = small_dynamics()
    for case in TRAJECTORY:
        lo, hi = trajectory_reference(m, case, torch.float32), trajectory_reference(m, case, torch.float64)
        out['trajectory'][case] = max(rel_err(lo[k], hi[k]) for k in hi)
    return out


if __name__ == '__main__':
    got = measure()
    print('E32_NS = {')
    for k, v in got['ns'].items():
        print(f'    {k!r}: {1.25 * v:.2e},')
    print('}')
    print('E32_ADAM =', {k: float(f'{1.25 * v:.2e}') for k, v in got['adam'].items()})
    print('E32_SUMSQ =', float(f'{1.25 * got["sumsq"]:.2e}'))
    print('E32_TRAJECTORY =', {k: float(f'{1.25 * v:.2e}') for k, v in got['trajectory'].items()})
