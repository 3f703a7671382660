"""Emulation of the arithmetic contract of the bf16-product form of the tiled attention core of the training path (csrc/attn_tiled_bf16.hip,
DESIGN.md 18), for tests/test_train_attn_bf16_host.py: what the kernels compute, rounding by rounding, written out by hand.  It takes the
arguments of tests/train_core_ref.py's self_core / cross_core and returns the same dict of problem-major outputs.

    pre    fp32: value-residual mix, k' = k / max(|k|, 1e-12) (gamma + 1) sqrt(dh), rotary on q and k', 1/|k|, 1/|v|, sigmoids; then the bf16
           images q^, k^', v^ (round to nearest even)
    fwd    S = q^ k^'^T (exact products, wide accumulate), / sqrt(dh), soft clamp, visibility; the keys a tile at a time with a running maximum;
           p = exp(s - m_running); the row sum takes p, the product p^ v^ the rounded p; o = sum / l; lse = m + log l; belief off the query's
           own UNROUNDED v row; gate
    dprep  gate and belief backward as the fp32 core; dO^ = bf16(dO); delta_i = sum_f dO^_if o_if
    dq/dkv S again from the images; P = exp(s_clamped - lse); dP = dO^ v^^T; dS = P (dP - delta) (1 - tanh^2) / sqrt(dh); P^, dS^ rounded;
           dv = P^^T dO^, dq' = dS^ k^', dk' = dS^^T q^
    post   transposed rotary, key-norm backward, value-mix backward, d gamma partial: on the unrounded planes

This is NOT autograd through a rounded forward: the backward is the kernels' (P recomputed from the saved lse, delta from the rounded dO, the
rounded P and dS as operands).  `rounding=False` takes every rounding out: the result is then the exact reference (to float64 rounding),
which the host test asserts.  `dtype` is the precision of everything that is fp32 in the kernels; `tile` the keys per online-softmax step."""
import math

import torch

import train_core_ref as R

# the largest train_core_ref.problem_err of this emulation against the exact float64 reference over the core-1 cases of train_core_cases and
# the four variants (tile 64 / 16, float64 / float32), per family and tensor, measured by tests/test_train_attn_bf16_host.py (which lists the
# measured values and asserts these) and recorded with a quarter of headroom; the GPU bound of tests/test_gpu_train_attn_bf16.py is FACTOR x
E16 = {
    'self': dict(o3=4.02e-2, dq=3.18e-2, dk=2.44e-2, dv=6.83e-2, dgate=1.18e-1, dmix=5.39e-2, d_rv=1.33e-2, dgamma_part=4.70e-2),
    'cross': dict(o3=1.75e-2, dq=3.59e-2, dk=2.94e-2, dv=2.65e-2, dgate=1.36e-1, dgamma_part=2.97e-2),
}
FACTOR = 2


def family(c):
    return 'cross' if c['family'] == 'cross' else 'self'


def bound(fam, tensor):
    return FACTOR * E16[fam][tensor]


def _rnd(x, on):
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def _rot(t, inv_freq, transposed=False):
    if inv_freq is None:
        return t
    n, dh = t.shape[-2], t.shape[-1]
    ang = torch.arange(n, dtype=t.dtype).view(-1, 1) * inv_freq.view(1, -1)
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    if not transposed:
        return t * cos + torch.cat([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin
    u = t * sin
    return t * cos + torch.cat([u[..., dh // 2:], -u[..., :dh // 2]], -1)


def _core(q, k, v, gate_logit, gamma_g, mix_logit, rv, d_o3, dh, softclamp, num_special, belief, causal, inv_freq, tile, rounding):
    """q, d_o3 [G][H][nq][dh]; k, v, rv [G][H][nk][dh]; gate_logit [G][H][nq]; mix_logit [G][H][nk]; gamma_g [G][H][dh]"""
    nq, nk = q.shape[2], k.shape[2]
    scale = 1 / math.sqrt(dh)
    # ---- pre
    mx = torch.sigmoid(mix_logit).unsqueeze(-1) if rv is not None else None
    vm = v + mx * (rv - v) if rv is not None else v
    kinv = 1 / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    kh = k * kinv
    sc = ((gamma_g + 1) * math.sqrt(dh)).unsqueeze(2)
    qr, kn = _rot(q, inv_freq), _rot(kh * sc, inv_freq)
    vinv = 1 / vm.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    gt = torch.sigmoid(gate_logit).unsqueeze(-1)
    qb, kb, vb = _rnd(qr, rounding), _rnd(kn, rounding), _rnd(vm, rounding)
    i, j = torch.arange(nq).view(-1, 1), torch.arange(nk).view(1, -1)
    fs = nk - num_special
    hidden = (i < fs) & (j >= fs)
    if causal:
        hidden = hidden | (j > i)

    def clamped(s):
        s = s * scale
        th = torch.tanh(s / softclamp) if softclamp > 0 else torch.zeros_like(s)
        return (th * softclamp if softclamp > 0 else s), th
    # ---- fwd: online softmax over tiles of keys
    m = torch.full(q.shape[:3] + (1,), -math.inf, dtype=q.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for j0 in range(0, nk, tile):
        s, _ = clamped(qb @ kb[:, :, j0:j0 + tile].transpose(-1, -2))
        s = s.masked_fill(hidden[:, j0:j0 + tile], -math.inf)
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.where(mn > -math.inf, torch.exp(m - mn), torch.zeros_like(m))
        p = torch.where(s > -math.inf, torch.exp(s - mn), torch.zeros_like(s))
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + _rnd(p, rounding) @ vb[:, :, j0:j0 + tile]
        m = mn
    o = o / l
    lse = m + torch.log(l)
    use_belief = bool(belief)
    vn = vm * vinv
    sdot = (o * vn).sum(-1, keepdim=True) if use_belief else None
    o2 = o - sdot * vn if use_belief else o
    out = {'o3': o2 * gt}
    if d_o3 is None:
        return out
    # ---- dprep
    out['dgate'] = ((d_o3 * o2).sum(-1, keepdim=True) * gt * (1 - gt)).squeeze(-1)
    d2 = d_o3 * gt
    dO, dvdir = d2, torch.zeros_like(vm)
    if use_belief:
        c2 = (d2 * vn).sum(-1, keepdim=True)
        dO = d2 - c2 * vn
        dvn = -(sdot * d2 + c2 * o)
        dvdir = (dvn - (dvn * vn).sum(-1, keepdim=True) * vn) * vinv
    dOb = _rnd(dO, rounding)
    delta = (dOb * o).sum(-1, keepdim=True)
    # ---- dq / dkv
    sc_, th = clamped(qb @ kb.transpose(-1, -2))
    P = torch.where(hidden, torch.zeros_like(sc_), torch.exp(sc_ - lse))
    dP = dOb @ vb.transpose(-1, -2)
    dS = P * (dP - delta)
    if softclamp > 0:
        dS = dS * (1 - th * th)
    dS = dS * scale
    Pb, dSb = _rnd(P, rounding), _rnd(dS, rounding)
    dv = Pb.transpose(-1, -2) @ dOb
    dqr, dknr = dSb @ kb, dSb.transpose(-1, -2) @ qb
    # ---- post
    out['dq'] = _rot(dqr, inv_freq, transposed=True)
    dkn = _rot(dknr, inv_freq, transposed=True)
    out['dgamma_part'] = (dkn * kh).sum(2) * math.sqrt(dh)
    dkh = dkn * sc
    out['dk'] = (dkh - (dkh * kh).sum(-1, keepdim=True) * kh) * kinv
    dv = dv + dvdir
    if rv is not None:
        out['dmix'] = ((dv * (rv - v)).sum(-1, keepdim=True) * mx * (1 - mx)).squeeze(-1)
        out['dv'], out['d_rv'] = dv * (1 - mx), dv * mx
    else:
        out['dv'] = dv
        if mix_logit is not None:
            out['dmix'] = torch.zeros_like(mix_logit)
    return out


def self_core(proj, ldp, rv, gamma, d_o3, *, groups, items, heads, dh, softclamp, num_special, belief, g_inner, g_outer_stride, item_stride,
              causal, inv_freq, dtype=torch.float64, tile=64, rounding=True):
    hd = heads * dh
    rows = R.self_rows(groups, items, g_inner, g_outer_stride, item_stride)
    c = lambda t: None if t is None else t.to(dtype)
    proj, rv, gamma, d_o3, inv_freq = c(proj), c(rv), c(gamma), c(d_o3), c(inv_freq)
    q, k, v = (R.take(proj, ldp, rows, col, heads, dh) for col in (0, hd, 2 * hd))
    gate, mix = R.take(proj, ldp, rows, 3 * hd, heads, 0), R.take(proj, ldp, rows, 3 * hd + R.hp4_of(heads), heads, 0)
    r = None if rv is None else R.take(rv, hd, rows, 0, heads, dh)
    d = None if d_o3 is None else R.take(d_o3, hd, rows, 0, heads, dh)
    return _core(q, k, v, gate, gamma.view(1, heads, dh).expand(groups, heads, dh), mix, r, d, dh, softclamp, num_special, belief, causal, inv_freq,
                 tile, rounding)


def cross_core(projq, ldq, projk, ldk, gamma, d_o3, *, groups, nq, nk, heads, dh, item_major, softclamp, dtype=torch.float64, tile=64, rounding=True):
    hd = heads * dh
    qrows, krows = R.cross_q_rows(groups, nq), R.cross_k_rows(groups, nk, item_major)
    c = lambda t: None if t is None else t.to(dtype)
    projq, projk, gamma, d_o3 = c(projq), c(projk), c(gamma), c(d_o3)
    q, gate = R.take(projq, ldq, qrows, 0, heads, dh), R.take(projq, ldq, qrows, hd, heads, 0)
    k, v = R.take(projk, ldk, krows, 0, heads, dh), R.take(projk, ldk, krows, hd, heads, dh)
    d = None if d_o3 is None else R.take(d_o3, hd, qrows, 0, heads, dh)
    return _core(q, k, v, gate, gamma.view(1, heads, dh).expand(groups, heads, dh), None, None, d, dh, softclamp, 0, 0, 0, None, tile, rounding)


def evaluate(c, d, dtype=torch.float64, tile=64, rounding=True):
    """the emulation on the inputs `d` of case `c` of tests/train_core_cases.py"""
    import train_core_cases as K
    if c['family'] == 'cross':
        ldq, ldk = K.cross_lds(c)
        return cross_core(d['projq'], ldq, d['projk'], ldk, d['gamma'], d['d_o3'], groups=c['groups'], nq=c['nq'], nk=c['nk'], heads=c['heads'], dh=c['dh'],
                          item_major=c['item_major'], softclamp=c['clamp'], dtype=dtype, tile=tile, rounding=rounding)
    return self_core(d['proj'], K.self_ldp(c), d['rv'], d['gamma'], d['d_o3'], groups=c['groups'], items=c['items'], heads=c['heads'], dh=c['dh'],
                     softclamp=c['clamp'], num_special=c['ns'], belief=c['belief'], g_inner=c['g_inner'], g_outer_stride=c['outer'], item_stride=c['item'],
                     causal=int(c['geo'] == 'time'), inv_freq=d['inv_freq'], dtype=dtype, tile=tile, rounding=rounding)
