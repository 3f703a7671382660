"""The contract of MuonAdamAtan2 (dreamer4_amd/optim.py) restated in plain torch, dtype-generic: evaluated in float64 it is the
reference of the GPU tests, evaluated in float32 on the CPU it measures E32 (tests/muon_cases.py).  `adam_atan2_pytorch` is absent here, so this
file IS the pinned arithmetic; nothing in it calls the package."""
import math

import torch

COEFS = (3.4445, -4.7750, 2.0315)


def newton_schulz(u, steps=5, coefs=COEFS, eps=1e-7):
    """X0 = u / max(|u|_F, eps) oriented rows <= cols; steps x (A = X X^T, B = b A + c A A, X <- a X + B X); oriented back."""
    a, b, c = coefs
    transposed = u.shape[0] > u.shape[1]
    X = u.t() if transposed else u
    X = X / max(float(torch.linalg.norm(X)), eps)
    for _ in range(steps):
        A = X @ X.t()
        B = b * A + c * (A @ A)
        X = a * X + B @ X
    return (X.t() if transposed else X).contiguous()


def update_scale(kind, r, c):
    return {'spectral': math.sqrt(max(1., r / c)), 'match_rms_adam': 0.2 * math.sqrt(max(r, c)), 'none': 1.}[kind]


def clip_coef(grads, max_grad_norm):
    """min(1, max_grad_norm / (global L2 norm + 1e-6)); 1 without a bound"""
    if max_grad_norm is None:
        return 1.
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return min(1., max_grad_norm / (norm + 1e-6))


def muon_step(W, g, m, *, lr, weight_decay=0., beta=0.95, nesterov=True, steps=5, coefs=COEFS, eps=1e-7, scale='spectral'):
    """-> (W', m')"""
    m = torch.lerp(m, g, 1. - beta)
    u = torch.lerp(g, m, beta) if nesterov else m
    X = newton_schulz(u, steps, coefs, eps)
    return W * (1. - lr * weight_decay) - lr * update_scale(scale, *W.shape) * X, m


def adam_atan2_step(W, g, m, v, t, *, lr, betas=(0.9, 0.99), weight_decay=0., a=1.27, b=1.):
    """-> (W', m', v'); t counts from 1"""
    b1, b2 = betas
    m = torch.lerp(m, g, 1. - b1)
    v = torch.lerp(v, g * g, 1. - b2)
    W = W * (1. - lr * weight_decay) - lr * a * torch.atan2(m / (1. - b1 ** t), b * torch.sqrt(v / (1. - b2 ** t)))
    return W, m, v


def optimiser_trajectory(params, muon_names, grads_per_step, dtype, *, lr, muon_lr=None, betas=(0.9, 0.99), weight_decay=0., a=1.27, b=1.,
                         muon_beta=0.95, muon_steps=5, muon_coefs=COEFS, muon_eps=1e-7, muon_nesterov=True, muon_update_scale='spectral',
                         max_grad_norm=None):
    """MuonAdamAtan2.step() once per entry of grads_per_step ({name: gradient or None}) on copies of `params` ({name: tensor}) in `dtype`.
    Names in muon_names step with Muon, the others with Adam-atan2; a None gradient skips the parameter (its step count does not advance)."""
    W = {k: p.detach().to(dtype).clone() for k, p in params.items()}
    M = {k: torch.zeros_like(p) for k, p in W.items()}
    V = {k: torch.zeros_like(p) for k, p in W.items()}
    T = {k: 0 for k in W}
    for grads in grads_per_step:
        live = {k: g.to(dtype) for k, g in grads.items() if g is not None}
        coef = clip_coef(list(live.values()), max_grad_norm)
        for k, g in live.items():
            g = g * coef
            T[k] += 1
            if k in muon_names:
                W[k], M[k] = muon_step(W[k], g, M[k], lr=muon_lr or lr, weight_decay=weight_decay, beta=muon_beta, nesterov=muon_nesterov, steps=muon_steps,
                                       coefs=muon_coefs, eps=muon_eps, scale=muon_update_scale)
            else:
                W[k], M[k], V[k] = adam_atan2_step(W[k], g, M[k], V[k], T[k], lr=lr, betas=betas, weight_decay=weight_decay, a=a, b=b)
    return W
