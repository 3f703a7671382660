"""Shapes, inputs and tolerances of the tests of MuonAdamAtan2's bf16 products (tests/test_muon_bf16_host.py, test_gpu_muon_bf16_ops.py,
test_gpu_muon_bf16.py).

E16[(name, steps)] is the largest muon_cases.rel_err of the emulated contract (tests/muon_bf16_ref.py) against the exact float64 muon_ref.newton_schulz
over four variants of the emulation: products in float64 and in float32, each over the whole K and accumulated in chunks of 32 k.  Measured by
`python tests/muon_bf16_cases.py`, recorded below with 25 % headroom; the GPU bound is FACTOR (2) x E16: the factor is room for the kernel's own
accumulation order (the variants differ by at most 1.2x among themselves).

`lowrank` at 5 steps is judged on what its input determines.  Its rank-4 input carries 1e-3 noise whose directions five iterations amplify to O(1), and
the bf16 roundings re-draw them: the emulation alone is 0.6 away from float64 element-wise.  The bound there is on P(X) = U4 U4^T X V4 V4^T, with U4, V4
the leading singular vectors of the float64 input, and the output must be finite."""
import torch

import muon_bf16_ref as E
import muon_cases as MC
import muon_ref as R

FACTOR = 2.
NS_SHAPES = dict(MC.NS_SHAPES, three_tiles=(260, 520))      # three 128-tile rows: mirrored tiles (0,1), (0,2), (1,2); five k-tiles of 128 in gram
NS_STEPS = (1, 5)
VARIANTS = tuple((dtype, chunk) for dtype in (torch.float64, torch.float32) for chunk in (None, 32))
PROJECTED = {('lowrank', 5)}


def ns_input(name):
    if name in MC.NS_SHAPES:
        return MC.ns_input(name)
    r, c = NS_SHAPES[name]
    return torch.randn(r, c, generator=torch.Generator().manual_seed(2000 + sorted(NS_SHAPES).index(name)))


def projector(name):
    """X -> U4 U4^T X V4 V4^T (float64) for the rank-4 part of the input"""
    U, _, Vh = torch.linalg.svd(ns_input(name).double(), full_matrices=False)
    U4, V4 = U[:, :4], Vh[:4].t()
    return lambda X: U4 @ (U4.t() @ X.double() @ V4) @ V4.t()


def ns_err(name, steps, got, exact):
    """the error a case is judged by: rel_err, on the projected matrices for the PROJECTED cases"""
    if (name, steps) in PROJECTED:
        P = projector(name)
        return MC.rel_err(P(got), P(exact))
    return MC.rel_err(got, exact)


# measured by `python tests/muon_bf16_cases.py` (largest of the four variants against float64), x 1.25
E16_NS = {
    ('tiny', 1): 4.53e-03, ('tiny', 5): 4.19e-02,
    ('square', 1): 4.26e-03, ('square', 5): 2.50e-02,
    ('ragged', 1): 4.52e-03, ('ragged', 5): 3.43e-02,
    ('tall', 1): 5.44e-03, ('tall', 5): 2.66e-02,
    ('odd_ld', 1): 5.08e-03, ('odd_ld', 5): 3.43e-02,
    ('lowrank', 1): 4.46e-03, ('lowrank', 5): 7.53e-03,
    ('multi', 1): 4.88e-03, ('multi', 5): 2.57e-02,
    ('two_tiles', 1): 5.99e-03, ('two_tiles', 5): 2.29e-02,
    ('three_tiles', 1): 6.12e-03, ('three_tiles', 5): 2.39e-02,
}
# the emulation in place of muon_ref.newton_schulz in the three-step trajectory of muon_cases.TRAJECTORY, Muon-group parameters, x 1.25
E16_TRAJECTORY = {'nesterov_spectral_clip': 1.73e-03, 'plain_rms': 8.39e-03}


def measure_ns(name, steps):
    u = ns_input(name)
    exact = R.newton_schulz(u.double(), steps)
    return max(ns_err(name, steps, E.newton_schulz(u.to(dtype), steps, chunk=chunk), exact) for dtype, chunk in VARIANTS)


def muon_names(model):
    names = {id(p): k for k, p in model.named_parameters()}
    return {names[id(p)] for p in model.muon_parameters()}


def measure_trajectory(case):
    """the emulated trajectory against the float64 one, over the Muon-group parameters, relative to each tensor's max-abs"""
    m = MC.small_dynamics()
    hi = MC.trajectory_reference(m, case, torch.float64)
    worst = 0.
    for dtype, chunk in VARIANTS:
        with E.in_place_of_newton_schulz(chunk=chunk):
            lo = MC.trajectory_reference(m, case, dtype)
        worst = max(worst, max(MC.rel_err(lo[k], hi[k]) for k in muon_names(m) if k in hi))
    return worst


if __name__ == '__main__':
    print('E16_NS = {')
    for name in NS_SHAPES:
        print('    ' + ' '.join(f'{(name, steps)!r}: {1.25 * measure_ns(name, steps):.2e},' for steps in NS_STEPS))
    print('}')
    print('E16_TRAJECTORY =', {case: float(f'{1.25 * measure_trajectory(case):.2e}') for case in MC.TRAJECTORY})
