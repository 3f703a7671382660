"""The arithmetic contract of MuonAdamAtan2(muon_products='bf16') emulated by hand in plain torch, dtype-generic: the Newton-Schulz
iteration of tests/muon_ref.py with every rounding the contract names put in through torch.bfloat16.

    X0 = bf16(u * 1 / max(|u|_F, eps))                  scaled in the working dtype, rounded once
    steps x:  A = bf16(X X^T);  B = bf16(b A + c (A A^T));  X <- bf16(a X + B X)

The products take the (bf16-valued) operands in the working dtype, over the whole K or accumulated in chunks of `chunk` k (the kernel's k-tiles add up
in a fixed order; the order inside an MFMA is the hardware's).  With round=False no rounding is left and the function IS muon_ref.newton_schulz
(tests/test_muon_bf16_host.py holds it to 1e-12 in float64).  Nothing here calls the package."""
import contextlib

import torch

import muon_ref as R


def rb(x, on=True):
    """round to bf16 (nearest even) and widen back"""
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def product(P, Q, chunk=None):
    """P Q^T for P [m][k], Q [n][k]: whole K, or partial products of `chunk` k added in order"""
    if chunk is None:
        return P @ Q.t()
    acc = torch.zeros(P.shape[0], Q.shape[0], dtype=P.dtype)
    for k0 in range(0, P.shape[1], chunk):
        acc = acc + P[:, k0:k0 + chunk] @ Q[:, k0:k0 + chunk].t()
    return acc


def newton_schulz(u, steps=5, coefs=R.COEFS, eps=1e-7, *, round=True, chunk=None):
    a, b, c = coefs
    transposed = u.shape[0] > u.shape[1]
    X = u.t() if transposed else u
    X = rb(X * (1. / max(float(torch.linalg.norm(X)), eps)), round)
    for _ in range(steps):
        A = rb(product(X, X, chunk), round)
        B = rb(b * A + c * product(A, A, chunk), round)                     # A A as A A^T: A is symmetric
        X = rb(a * X + product(B, X.t().contiguous(), chunk), round)        # B X = B (X^T)^T: the kernel reads the transposed image of X
    return (X.t() if transposed else X).contiguous()


@contextlib.contextmanager
def in_place_of_newton_schulz(**kw):
    """muon_ref.muon_step / optimiser_trajectory with the emulation as their Newton-Schulz (muon_ref itself stays as it is)"""
    keep = R.newton_schulz
    R.newton_schulz = lambda u, steps=5, coefs=R.COEFS, eps=1e-7: newton_schulz(u, steps, coefs, eps, **kw)
    try:
        yield
    finally:
        R.newton_schulz = keep
