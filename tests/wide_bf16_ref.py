"""Emulation of the arithmetic contract of the bf16-product wide attention core (csrc/attn_wide_bf16.hip: wide_attn_bf16_kernel<DH>,
DESIGN.md 16) on logical tensors, built on attn_core_ref.prep_kv / _belief:

  k' and v' in `dtype`, then rounded through torch.bfloat16; q rounded through torch.bfloat16; S = q^ k^'^T; scale, soft clamp and the
  special-token rule in `dtype`; the keys walked `tile` at a time with a running maximum; p = exp(s - m_running) rounded through
  torch.bfloat16 for p^ v^', the row sum from the unrounded p; belief projection against the query's own UNROUNDED v' row; head gate.

`dtype` float64 is the contract itself, float32 the same at the kernel's precision; `tile` 64 is the kernel's key tile (16 shows how
much the result depends on where the running maximum changes).  This is not the tolerance's reference: the GPU test compares against
the exact float64 attn_core_ref.small_attn_ref, and tests/test_wide_bf16_host.py measures how far this emulation is from it."""
import math

import torch

import attn_core_ref as R


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def wide_bf16_ref(q, k, v, gamma, gate=None, vres=None, mix=None, *, clamp, mask_special=0, belief=0, dtype=torch.float64, tile=64):
    """q [G or 1, H, nq, dh]; k, v, vres [G, H, nk, dh]; gamma [H, dh]; gate [G, H, nq]; mix [G, H, nk]  ->  [G, H, nq, dh]"""
    q, k, v, gamma, gate, vres, mix = R._to(dtype, q, k, v, gamma, gate, vres, mix)
    nq, dh, nk = q.shape[2], q.shape[3], k.shape[2]
    k, v = R.prep_kv(k, v, gamma[None, :, None, :], vres, mix, dh)
    qh, kh, vh = bf16(q), bf16(k), bf16(v)
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(dh)
    s = s.expand(k.shape[0], -1, -1, -1).clone()
    if clamp > 0:
        s = clamp * torch.tanh(s / clamp)
    if mask_special > 0:                     # the ordinary queries do not see the trailing special keys
        s[:, :, :nq - mask_special, nk - mask_special:] = -math.inf
    m = torch.full(s.shape[:-1], -math.inf, dtype=dtype)
    l = torch.zeros(s.shape[:-1], dtype=dtype)
    o = torch.zeros(*s.shape[:-1], dh, dtype=dtype)
    for j0 in range(0, nk, tile):
        st = s[..., j0:j0 + tile]
        mn = torch.maximum(m, st.max(-1).values)             # (key 0 is visible to every query: finite from the first tile on)
        alpha = torch.exp(m - mn)
        p = torch.exp(st - mn[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + bf16(p) @ vh[..., j0:j0 + tile, :]
        m = mn
    o = o / l[..., None]
    if belief:
        o = R._belief(o, v)
    if gate is not None:
        o = o * torch.sigmoid(gate)[..., None]
    return o
