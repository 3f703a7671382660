"""Plain torch restatement of one attention core of the training path (csrc/backward.hip: attn_bwd_kernel / xattn_bwd_kernel; csrc/attn_tiled.hip),
self and cross, for tests/test_gpu_train_cores.py and tests/test_train_cores_host.py.  A second, independent statement: it shares nothing with
oracle/ and is evaluated in float64 (float32 for the E32 measurement of train_core_cases.py), gradients by autograd.

It takes what the kernels take: flat [rows][ld] buffers and the row rule of AttnBwdArgs / XAttnArgs, so the geometry is part of what is checked.
    self   row of item j of group g = (g // g_inner) * g_outer_stride + g % g_inner + j * item_stride
           columns of proj: q @ 0, k @ hd, v @ 2hd, gate logit @ 3hd + head, mix logit @ 3hd + hp4 + head  (hd = heads * dh, hp4 = heads rounded up to 4)
    cross  query i of group g: row g * nq + i of projq (q @ 0, gate logit @ hd + head); key j of group g: row g * nk + j of projk, or j * groups + g
           when item_major (k @ 0, v @ hd)
The operation: q as given; k L2-normalised (eps 1e-12) times (gamma + 1) sqrt(dh); v mixed with the residual by the sigmoid of the mix logit;
rotary (half split) on q and on the scaled key at positions 0 .. items - 1; sim / sqrt(dh); tanh soft clamp when softclamp > 0; ordinary queries
do not see the last num_special items, causal j <= i; softmax; P V; the belief projection off the normalised mixed value of the query's own
row; the head gate.  Cross: no residual, rotary, mask or belief.

Outputs are problem major, [groups][heads][...]: o3, dq, dk, dv [G][H][n][dh]; dgate, dmix [G][H][n]; d_rv [G][H][n][dh]; dgamma_part [G][H][dh]
(the gradient of gamma through group g's keys alone, which is what the kernels write: sqrt(dh) is inside it)."""
import math

import torch

# each keyword breaks one thing.  The last three were added for the one-key problems (items 1, one context key): their softmax is constant,
# so none of the others can move their outputs.
MUTATIONS = ('gamma_only', 'no_belief', 'no_vres', 'mask_row', 'causal_strict', 'k_unrotated', 'no_clamp', 'scale64', 'item_major_swapped',
             'g_inner_ignored', 'no_gate', 'v_from_k', 'ld_min')


def hp4_of(heads):
    return (heads + 3) // 4 * 4


def self_rows(groups, items, g_inner, g_outer_stride, item_stride):
    g = torch.arange(groups).view(-1, 1)
    return (g // g_inner) * g_outer_stride + g % g_inner + torch.arange(items).view(1, -1) * item_stride


def cross_q_rows(groups, nq):
    return torch.arange(groups).view(-1, 1) * nq + torch.arange(nq).view(1, -1)


def cross_k_rows(groups, nk, item_major):
    g, j = torch.arange(groups).view(-1, 1), torch.arange(nk).view(1, -1)
    return j * groups + g if item_major else g * nk + j


def take(buf, ld, rows, col, heads, width):
    """columns col .. col + heads * width of the rows `rows` [G][n] of the flat [.][ld] buffer -> [G][heads][n][width] (width 0: a scalar per head)"""
    x = buf.view(-1, ld)[rows][..., col:col + heads * max(width, 1)]
    G, n = rows.shape
    if width == 0:
        return x.permute(0, 2, 1).contiguous()
    return x.view(G, n, heads, width).permute(0, 2, 1, 3).contiguous()


def _rotate(t, inv_freq):
    n, dh = t.shape[-2], t.shape[-1]
    ang = torch.arange(n, dtype=t.dtype).view(-1, 1) * inv_freq.view(1, -1)           # (formed in the evaluation's precision, as the kernels form it in float32)
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    half = torch.cat([-t[..., dh // 2:], t[..., :dh // 2]], -1)
    return t * cos + half * sin


def _attend(q, k, v, gate_logit, gamma_g, mix_logit, rv, dh, softclamp, num_special, belief, causal, inv_freq, mut):
    """q [G][H][nq][dh], k / v / rv [G][H][nk][dh], gate_logit [G][H][nq], mix_logit [G][H][nk], gamma_g [G][H][dh] -> o3 [G][H][nq][dh]"""
    nq, nk = q.shape[2], k.shape[2]
    if rv is not None and 'no_vres' not in mut:
        v = v + torch.sigmoid(mix_logit).unsqueeze(-1) * (rv - v)
    kh = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    g = gamma_g if 'gamma_only' in mut else gamma_g + 1
    kn = kh * (g * math.sqrt(dh)).unsqueeze(2)
    if inv_freq is not None:
        q = _rotate(q, inv_freq)
        if 'k_unrotated' not in mut:
            kn = _rotate(kn, inv_freq)
    sim = q @ kn.transpose(-1, -2) * (0.125 if 'scale64' in mut else 1 / math.sqrt(dh))
    if softclamp > 0 and 'no_clamp' not in mut:
        sim = torch.tanh(sim / softclamp) * softclamp
    i, j = torch.arange(nq).view(-1, 1), torch.arange(nk).view(1, -1)
    fs = nk - num_special
    hidden = (i < fs) & (j >= fs)
    if 'mask_row' in mut:
        hidden = hidden & (i != fs - 1)
    if causal:
        hidden = hidden | (torch.where(i > 0, j >= i, j > i) if 'causal_strict' in mut else j > i)
    sim = sim.masked_fill(hidden, -math.inf)
    o = torch.softmax(sim, -1) @ v
    if belief and 'no_belief' not in mut:
        vn = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        o = o - (o * vn).sum(-1, keepdim=True) * vn
    return o if 'no_gate' in mut else o * torch.sigmoid(gate_logit).unsqueeze(-1)


def _grads(o3, d_o3, leaves):
    present = {n: t for n, t in leaves.items() if t is not None}
    g = torch.autograd.grad(o3, list(present.values()), d_o3, allow_unused=True)
    return {n: (torch.zeros_like(t) if x is None else x) for (n, t), x in zip(present.items(), g)}


def self_core(proj, ldp, rv, gamma, d_o3, *, groups, items, heads, dh, softclamp, num_special, belief, g_inner, g_outer_stride, item_stride,
              causal, inv_freq, dtype=torch.float64, mut=()):
    """proj flat [rows * ldp], rv / d_o3 flat [rows * hd] (or None), gamma [heads * dh], inv_freq [dh / 2] or None -> dict of outputs"""
    hd = heads * dh
    rows = self_rows(groups, items, 1, items, 1) if 'g_inner_ignored' in mut else self_rows(groups, items, g_inner, g_outer_stride, item_stride)
    c = lambda t: None if t is None else t.to(dtype)
    proj, rv, gamma, d_o3, inv_freq = c(proj), c(rv), c(gamma), c(d_o3), c(inv_freq)
    ld = 3 * hd + hp4_of(heads) + heads if 'ld_min' in mut else ldp
    if ld != ldp:
        proj = proj[:proj.numel() // ld * ld]
    leaf = lambda t: t.clone().requires_grad_(True)
    q, k = leaf(take(proj, ld, rows, 0, heads, dh)), leaf(take(proj, ld, rows, hd, heads, dh))
    v = leaf(take(proj, ld, rows, hd if 'v_from_k' in mut else 2 * hd, heads, dh))
    gate, mix = leaf(take(proj, ld, rows, 3 * hd, heads, 0)), leaf(take(proj, ld, rows, 3 * hd + hp4_of(heads), heads, 0))
    r = None if rv is None else leaf(take(rv, hd, rows, 0, heads, dh))
    gamma_g = leaf(gamma.view(1, heads, dh).expand(groups, heads, dh))
    o3 = _attend(q, k, v, gate, gamma_g, mix, r, dh, softclamp, num_special, belief, causal, inv_freq, mut)
    out = {'o3': o3.detach()}
    if d_o3 is not None:
        g = _grads(o3, take(d_o3, hd, rows, 0, heads, dh), dict(dq=q, dk=k, dv=v, dgate=gate, dmix=mix, d_rv=r, dgamma_part=gamma_g))
        out.update(g)
    return out


def cross_core(projq, ldq, projk, ldk, gamma, d_o3, *, groups, nq, nk, heads, dh, item_major, softclamp, dtype=torch.float64, mut=()):
    hd = heads * dh
    qrows = cross_q_rows(groups, nq)
    krows = cross_k_rows(groups, nk, (not item_major) if 'item_major_swapped' in mut else item_major)
    c = lambda t: None if t is None else t.to(dtype)
    projq, projk, gamma, d_o3 = c(projq), c(projk), c(gamma), c(d_o3)
    lq, lk = (hd + heads, 2 * hd) if 'ld_min' in mut else (ldq, ldk)
    projq, projk = projq[:projq.numel() // lq * lq], projk[:projk.numel() // lk * lk]
    leaf = lambda t: t.clone().requires_grad_(True)
    q, gate = leaf(take(projq, lq, qrows, 0, heads, dh)), leaf(take(projq, lq, qrows, hd, heads, 0))
    k, v = leaf(take(projk, lk, krows, 0, heads, dh)), leaf(take(projk, lk, krows, 0 if 'v_from_k' in mut else hd, heads, dh))
    gamma_g = leaf(gamma.view(1, heads, dh).expand(groups, heads, dh))
    o3 = _attend(q, k, v, gate, gamma_g, None, None, dh, softclamp, 0, 0, 0, None, mut)
    out = {'o3': o3.detach()}
    if d_o3 is not None:
        out.update(_grads(o3, take(d_o3, hd, qrows, 0, heads, dh), dict(dq=q, dk=k, dv=v, dgate=gate, dgamma_part=gamma_g)))
    return out


def problem_err(got, ref, zero_scale=None):
    """got, ref [G][H][...]: the largest error of a (group, head) problem relative to that problem's max |ref|, floored at 1e-3 of the tensor's
    max |ref|; a tensor whose reference is identically zero is measured against zero_scale.  -> (per problem, per tensor)"""
    G, H = ref.shape[:2]
    d = (got.double() - ref.double()).abs().reshape(G * H, -1).amax(1)
    r = ref.double().abs().reshape(G * H, -1).amax(1)
    top = r.max().item()
    if top == 0:
        assert zero_scale, 'an identically zero reference needs a scale'
        top, r = zero_scale, torch.full_like(r, zero_scale)
    return (d / r.clamp_min(1e-3 * top)).max().item(), (d.max() / top).item()


def errors(got, ref):
    """dict tensor -> (per-problem error, per-tensor error) over the tensors of ref; dq / dk / dgamma_part of a one-key problem are identically
    zero in the reference and are measured against max |dv| (train_core_cases.py)."""
    zs = ref['dv'].double().abs().max().item() if 'dv' in ref else None
    return {n: problem_err(got[n], ref[n], zs) for n in ref}
