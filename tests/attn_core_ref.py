"""Plain references of the inference attention cores (csrc/attn.hip: small_attn, pool_mix, the cached time decode), written from the
model's semantics on logical tensors — no strides, no tiling, no online softmax.  Every function takes a `dtype`: float64 is the reference
the GPU tests compare against, float32 the same code at the kernels' precision (its distance to float64 is the E32 the tolerance is
derived from, see attn_core_cases.py).

`mut` names deliberate mistakes (tests/test_attn_cores_host.py): the host test evaluates the float64 reference with each of them to show
that the inputs and the bound of the GPU tests can see such an error.  An empty `mut` is the correct operation."""
import math

import torch

MUTATIONS = ('drop_newest', 'drop_oldest', 'extra_key', 'mask_row', 'no_belief', 'no_vres', 'rot_off', 'scale64', 'gamma_only', 'no_rms', 'gate_row', 'rot_off_k')


def _to(dtype, *ts):
    return [None if t is None else t.to(dtype) for t in ts]


def prep_kv(k, v, gamma, vres, mix, dh, mut=()):
    """v' = v + sigmoid(mix) (vres - v);  k' = k / max(|k|, 1e-12) * (gamma + 1) * sqrt(dh).   k, v, vres [..., dh]; mix [...]"""
    if vres is not None and 'no_vres' not in mut:
        v = v + torch.sigmoid(mix)[..., None] * (vres - v)
    g = gamma if 'gamma_only' in mut else gamma + 1
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12) * g * math.sqrt(64 if 'scale64' in mut else dh)
    return k, v


def _belief(o, v_own):
    vn = v_own / v_own.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return o - (o * vn).sum(-1, keepdim=True) * vn


def small_attn_ref(q, k, v, gamma, gate=None, vres=None, mix=None, *, clamp, mask_special=0, belief=0, q_lo=0, q_hi=0, q_last=1,
                   dtype=torch.float64, mut=()):
    """q [G or 1, H, nq, dh]; k, v, vres [G, H, nk, dh]; gamma [H, dh]; gate [G, H, nq]; mix [G, H, nk]  ->  [G, H, nq_out, dh]"""
    q, k, v, gamma, gate, vres, mix = _to(dtype, q, k, v, gamma, gate, vres, mix)
    nq, dh, nk = q.shape[2], q.shape[3], k.shape[2]
    k, v = prep_kv(k, v, gamma[None, :, None, :], vres, mix, dh, mut)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.expand(k.shape[0], -1, -1, -1).clone()
    if clamp > 0:
        s = clamp * torch.tanh(s / clamp)
    n_ord, n_vis = nq, nk
    if mask_special > 0:                     # the ordinary queries do not see the trailing special keys
        n_ord = nq - mask_special + (1 if 'mask_row' in mut else 0)
        n_vis = nk - mask_special + (1 if 'extra_key' in mut else 0)
        s[:, :, :n_ord, n_vis:] = -math.inf
    if 'drop_newest' in mut:                 # the last key each row sees
        s[:, :, :n_ord, n_vis - 1] = -math.inf
        s[:, :, n_ord:, nk - 1] = -math.inf
    if 'drop_oldest' in mut:
        s[..., 0] = -math.inf
    o = torch.softmax(s, dim=-1) @ v
    if belief and 'no_belief' not in mut:
        o = _belief(o, v)
    if gate is not None:
        o = o * torch.sigmoid(gate)[..., None]
    if q_hi > 0:
        o = o[:, :, list(range(q_lo, q_hi)) + ([nq - 1] if q_last else [])]
    return o


def rotary(x, pos, inv_freq, dtype):
    """Rotate-half rotary: frequencies cat(f, f), halves dh / 2 wide.  x [..., dh]; pos broadcastable to x.shape[:-1].  The angle pos * f is
    formed in `dtype` (float32: as the kernels do)."""
    hw = x.shape[-1] // 2
    ang = pos.to(dtype)[..., None] * inv_freq[:hw].to(dtype)
    ang = torch.cat((ang, ang), dim=-1)
    rot = torch.cat((-x[..., hw:], x[..., :hw]), dim=-1)
    return x * torch.cos(ang) + rot * torch.sin(ang)


def time_append_ref(proj, vres, gamma, inv_freq, cache, *, t0, H, dh, dtype=torch.float64, mut=()):
    """proj [B, Tq, S, 3 hd + 2 H] (q | k | v | gate logits | mix logits); vres [B, Tq, S, hd]; gamma [H, dh];
    cache [2, cache_batch, cache_S, H, Tcap, dh] of `dtype`, rows t0 .. t0 + Tq - 1 of slots [:B, :S] written in place."""
    proj, vres, gamma = _to(dtype, proj, vres, gamma)
    B, Tq, S, _ = proj.shape
    hd = H * dh
    k = proj[..., hd:2 * hd].reshape(B, Tq, S, H, dh)
    v = proj[..., 2 * hd:3 * hd].reshape(B, Tq, S, H, dh)
    k, v = prep_kv(k, v, gamma, vres.reshape(B, Tq, S, H, dh), proj[..., 3 * hd + H:3 * hd + 2 * H], dh, mut)
    pos = t0 + torch.arange(Tq) + (1 if 'rot_off_k' in mut else 0)
    k = rotary(k, pos[None, :, None, None], inv_freq, dtype)
    cache[0, :B, :S, :, t0:t0 + Tq] = k.permute(0, 2, 3, 1, 4)
    cache[1, :B, :S, :, t0:t0 + Tq] = v.permute(0, 2, 3, 1, 4)
    return cache


def time_attn_ref(proj, inv_freq, cache, *, t0, H, dh, clamp, dtype=torch.float64, mut=()):
    """Causal attention of the Tq frames of `proj` over cache positions 0 .. t0 + tq, belief against the position's own value, head gates.
    -> [B, Tq, S, hd]"""
    proj, cache = _to(dtype, proj, cache)
    B, Tq, S, _ = proj.shape
    hd = H * dh
    q = proj[..., :hd].reshape(B, Tq, S, H, dh)
    pos = t0 + torch.arange(Tq)
    q = rotary(q, (pos + (1 if 'rot_off' in mut else 0))[None, :, None, None], inv_freq, dtype)
    gate = torch.sigmoid(proj[..., 3 * hd:3 * hd + H])
    out = torch.empty(B, Tq, S, H, dh, dtype=dtype)
    for tq in range(Tq):
        p = t0 + tq
        lo = 1 if 'drop_oldest' in mut else 0
        hi = p + 1 + (1 if 'extra_key' in mut else 0) - (1 if 'drop_newest' in mut else 0)
        K, V = cache[0, :B, :S, :, lo:hi], cache[1, :B, :S, :, lo:hi]         # [B, S, H, keys, dh]
        s = (K @ q[:, tq, :, :, :, None])[..., 0] / math.sqrt(dh)
        if clamp > 0:
            s = clamp * torch.tanh(s / clamp)
        o = (torch.softmax(s, dim=-1)[..., None, :] @ V)[..., 0, :]
        if 'no_belief' not in mut:
            o = _belief(o, cache[1, :B, :S, :, p])
        out[:, tq] = o * gate[:, tq, :, :, None]
    return out.reshape(B, Tq, S, hd)


def pool_mix_ref(q, x, gate_w, k, hid, gamma, *, eps, dtype=torch.float64, mut=()):
    """q [M, 4 * 64]; x [M, D]; gate_w [4, D]; k [L, M, 4 * 64]; hid [L, M, D]; gamma [4, 64]  ->  u [M, 4, D]"""
    q, x, gate_w, k, hid, gamma = _to(dtype, q, x, gate_w, k, hid, gamma)
    L, M, D = hid.shape
    kk, _ = prep_kv(k.reshape(L, M, 4, 64), None, gamma, None, None, 64, mut)
    s = (kk * q.reshape(1, M, 4, 64)).sum(-1) / 8.                           # [L, M, 4]
    if 'drop_newest' in mut:
        s[L - 1] = -math.inf
    if 'drop_oldest' in mut:
        s[0] = -math.inf
    p = torch.softmax(s, dim=0)
    hn = hid if 'no_rms' in mut else hid / torch.sqrt((hid * hid).mean(-1, keepdim=True) + eps)
    if 'gate_row' in mut:
        x = x.roll(1, dims=0) if M > 1 else hid[0]
    g = torch.sigmoid((x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)) @ gate_w.t())       # [M, 4]
    return g[..., None] * torch.einsum('lmh,lmd->mhd', p, hn)


def rel_err(a, b):
    """max |a - b| relative to max |b| (b: the reference)."""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()
