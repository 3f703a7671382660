"""Plain references of the learner's loss kernels (csrc/learn.hip: gae_kernel, policy_loss_kernel with the advantage statistics and the final
division, value_loss_kernel), as tests/test_gpu_learn_ops.py calls them alone through d4_gae_adv, d4_policy_loss and d4_hl_gauss_ce.  Logical
tensors only: no strides, no grids.  Every function takes a `dtype` (float64: the reference of the GPU tests; float32: the same code at the
kernels' precision, whose distance to float64 is the E32 of learn_cases.py).  Gradients come from autograd, never from a formula written here;
the Beta head uses torch.lgamma / torch.special.digamma.  Nothing is taken from oracle/restate.py: tests/test_learn_ops_host.py checks the two
against each other.

`mut` names deliberate mistakes (tests/test_learn_ops_host.py shows that the inputs and the bounds of the GPU tests can see each):
  GAE
    no_trunc        truncation ignored: the last step of a truncated trajectory is learnt from
    past_len        rewards and values read past `len`
    no_lam          lambda dropped from the recurrence
    gamma_wrong     gamma multiplies the reward instead of the next value
    defaults_inv    the null defaults inverted: null is_truncated read as not truncated, null terminals as terminal
    last_traj       the last trajectory not written
  policy
    kl_swap         the KL direction exchanged
    kl_no_grad      the KL term left out of the gradient
    kl_no_const     the per-row constant `- kl` of the forward KL's logit gradient dropped
    clip_pass       PPO: the gradient passed outside the clip band
    tie_rule        PPO: a tie of the two surrogates takes the clipped branch (no gradient inside the band)
    spo_no_quad     SPO: the quadratic term dropped
    gate_grad       the delight gate differentiated instead of detached
    gate_sign       the gate's argument with the other sign
    gate_raw_adv    the gate reads the raw advantage where it is normalised
    var_unmasked    the advantage variance taken over every row
    no_eps_clamp    the variance not clamped at eps
    pmpo_sign0      PMPO: an advantage of exactly 0 counted as negative (inert by construction: its weight |tanh 0| is 0; the host test asserts that)
    no_alpha        PMPO: the positive-to-negative weight dropped
    ent_sign        the entropy bonus with the other sign
    beta_ent_grad   the Beta entropy left out of the gradient
    beta_log1mx     the Beta log-prob with log(1 - x) in place of log x
    link_swap       the other link (softplus for exp, exp for softplus)
    no_max          the log-sum-exp without the max subtraction (evaluated in float32, where it overflows)
    last_row        the last row not written
    last_type       the last discrete action type left out of the joint log-prob and entropy
    last_cont       the last continuous action left out
    mask_ignored    the mask read as all ones
    count_unclamped the division by the mask count without the clamp at 1
  value
    no_clamp        the returns not clamped into the range
    no_z            HL-Gauss: the normaliser z dropped
    swap_lr         two-hot: the left and right weights exchanged
    side            two-hot: searchsorted from the right
    last_bin        the last bin left out
    last_row        the last row not written
    no_psum         the target's sum dropped from the gradient (softmax - target instead of softmax * sum(target) - target)
    mask_ignored, count_unclamped   as for the policy"""
import math

import torch
import torch.nn.functional as F

GAE_MUTATIONS = ('no_trunc', 'past_len', 'no_lam', 'gamma_wrong', 'defaults_inv', 'last_traj')
POLICY_MUTATIONS = ('kl_swap', 'kl_no_grad', 'kl_no_const', 'clip_pass', 'tie_rule', 'spo_no_quad', 'gate_grad', 'gate_sign', 'gate_raw_adv', 'var_unmasked',
                    'no_eps_clamp', 'pmpo_sign0', 'no_alpha', 'ent_sign', 'beta_ent_grad', 'beta_log1mx', 'link_swap', 'no_max', 'last_row', 'last_type',
                    'last_cont', 'mask_ignored', 'count_unclamped')
VALUE_MUTATIONS = ('no_clamp', 'no_z', 'swap_lr', 'side', 'last_bin', 'last_row', 'no_psum', 'mask_ignored', 'count_unclamped')


def err(got, want):
    """max |got - want| relative to max |want|; a reference that is zero everywhere asks for exact zeros; a NaN or infinity where the reference
    has none is an infinite error."""
    got, want = got.double(), want.double()
    if not torch.isfinite(got).all():
        return math.inf
    scale = want.abs().max().item() if want.numel() else 0.
    d = (got - want).abs().max().item() if want.numel() else 0.
    if scale == 0.:
        return 0. if d == 0. else math.inf
    return d / scale


def err_all(got, want):
    """Largest err over the named outputs of two results (a None reference is an output the call does not write)."""
    return max(err(got[k], w) for k, w in want.items() if w is not None)


# ------------------------------------------------------------------------------------------------------------------- GAE
def gae_ref(rewards, values, lens, is_truncated, terminals, gamma, lam, dtype=torch.float64, mut=()):
    """rewards, values [B, T]; lens int64 [B] / is_truncated bool [B] / terminals bool [B], each or None -> returns, adv, mask [B, T]."""
    B, T = rewards.shape
    r, v = rewards.to(dtype), values.to(dtype)
    inv = 'defaults_inv' in mut
    lens = torch.full((B,), T, dtype=torch.long) if lens is None else lens.long()
    trunc = torch.full((B,), not inv, dtype=torch.bool) if is_truncated is None else is_truncated.bool()
    term = torch.full((B,), inv, dtype=torch.bool) if terminals is None else terminals.bool()
    ar = torch.arange(T)
    in_len = ar < lens[:, None]
    if 'past_len' not in mut:
        r, v = torch.where(in_len, r, torch.zeros_like(r)), torch.where(in_len, v, torch.zeros_like(v))
    learn = ar < (lens - (0 if 'no_trunc' in mut else trunc.long()))[:, None]
    last = (lens - 1).clamp(min=0)[:, None]
    cont = (ar < last) & ~((ar == last) & term[:, None])
    m = cont.to(dtype)
    v_next = torch.cat([v[:, 1:], torch.zeros(B, 1, dtype=dtype)], 1)
    delta = (gamma * r + v_next * m - v) if 'gamma_wrong' in mut else (r + gamma * v_next * m - v)
    delta = torch.where(learn, delta, torch.zeros_like(delta))
    g = torch.zeros(B, dtype=dtype)
    out = torch.zeros(B, T, dtype=dtype)
    for t in range(T - 1, -1, -1):
        g = gamma * (1. if 'no_lam' in mut else lam) * m[:, t] * g + delta[:, t]
        out[:, t] = g
    returns = out + v
    res = dict(returns=returns, adv=returns - v, mask=learn.to(dtype))
    if 'last_traj' in mut:
        res = {k: torch.cat([x[:-1], torch.zeros_like(x[-1:])]) for k, x in res.items()}
    return res


# ------------------------------------------------------------------------------------------------------------------- policy loss
def beta_ab(raw, link):
    f = torch.exp if link == 'exp' else F.softplus
    return f(raw[..., 0]) + 1., f(raw[..., 1]) + 1.


def lbeta(a, b):
    return torch.lgamma(a) + torch.lgamma(b) - torch.lgamma(a + b)


def beta_log_prob(a, b, x, mut=()):
    lx = torch.log1p(-x) if 'beta_log1mx' in mut else torch.log(x)
    return (a - 1.) * lx + (b - 1.) * torch.log1p(-x) - lbeta(a, b)


def beta_entropy(a, b):
    dg = torch.special.digamma
    return lbeta(a, b) - (a - 1.) * dg(a) - (b - 1.) * dg(b) + (a + b - 2.) * dg(a + b)


def beta_kl(a1, b1, a2, b2):
    """KL(Beta(a1, b1) || Beta(a2, b2))"""
    dg = torch.special.digamma
    return lbeta(a2, b2) - lbeta(a1, b1) + (a1 - a2) * dg(a1) + (b1 - b2) * dg(b1) + (a2 - a1 + b2 - b1) * dg(a1 + b1)


def log_softmax(l, mut=()):
    if 'no_max' in mut:                     # the unstabilised sum at the kernel's precision: exp overflows float32 for a logit of 90
        return l - torch.log(torch.exp(l.float()).sum(-1, keepdim=True)).to(l.dtype)
    return l - torch.logsumexp(l, -1, keepdim=True)


def policy_terms(p, logits, cparams, dtype=torch.float64, mut=()):
    """The differentiable part: p holds the constants of one call (see policy_ref) -> loss and the per-row terms, lp, ratio, kls."""
    R = p['rows']
    sizes, nc = list(p['sizes']), p['nc']
    if 'last_type' in mut and len(sizes) > 1:
        sizes_used = len(sizes) - 1
    else:
        sizes_used = len(sizes)
    link = p['link']
    if 'link_swap' in mut:
        link = 'softplus' if link == 'exp' else 'exp'
    mask = torch.ones(R, dtype=dtype) if p['mask'] is None or 'mask_ignored' in mut else p['mask'].to(dtype)
    count = mask.sum() if 'count_unclamped' in mut else mask.sum().clamp(min=1.)
    raw_adv = p['adv'].to(dtype)
    adv = raw_adv
    if p['normalize']:
        cnt1 = mask.sum().clamp(min=1.)
        mean = (raw_adv * mask).sum() / cnt1
        var = ((raw_adv - mean) ** 2 * (torch.ones_like(mask) if 'var_unmasked' in mut else mask)).sum() / cnt1
        adv = (raw_adv - mean) / torch.sqrt(var if 'no_eps_clamp' in mut else var.clamp(min=p['eps']))
    lp = torch.zeros(R, dtype=dtype)
    old = torch.zeros(R, dtype=dtype)
    ent = torch.zeros(R, dtype=dtype)
    kls = []
    kl_on = p['objective'] == 2 and p['kl_w'] > 0
    rev = bool(p['reverse_kl']) != ('kl_swap' in mut)
    o = 0
    for i, n in enumerate(sizes):
        if i < sizes_used:
            ls = log_softmax(logits[:, o:o + n], mut)
            lp = lp + ls.gather(1, p['actions'][:, i:i + 1]).squeeze(1)
            old = old + p['old_lp'][:, i].to(dtype)
            ent = ent - (ls.exp() * ls).sum(-1)
            if kl_on:
                lo = log_softmax(p['old_logits'][:, o:o + n].to(dtype))
                kl = (lo.exp() * (lo - ls)).sum(-1) if rev else (ls.exp() * (ls - lo)).sum(-1)
                if 'kl_no_const' in mut and not rev:     # value kept, gradient + kl * softmax: the logit gradient p_j (l_j - lo_j) without its - kl
                    lse = torch.logsumexp(logits[:, o:o + n], -1)
                    kl = kl + kl.detach() * (lse - lse.detach())
                kls.append(kl)
        o += n
    ncu = nc - 1 if 'last_cont' in mut and nc > 0 and (nc > 1 or sizes) else nc
    for c in range(ncu):
        a, b = beta_ab(cparams[:, 2 * c:2 * c + 2], link)
        x = p['actions_cont'][:, c].to(dtype)
        lp = lp + beta_log_prob(a, b, x, mut)
        old = old + p['old_lp_cont'][:, c].to(dtype)
        h = beta_entropy(a, b)
        ent = ent + (h.detach() if 'beta_ent_grad' in mut else h)
        if kl_on:
            a2, b2 = beta_ab(p['old_cparams'][:, c].to(dtype), link)
            kls.append(beta_kl(a2, b2, a, b) if rev else beta_kl(a, b, a2, b2))
    gate = torch.ones(R, dtype=dtype)
    if p['use_gate']:
        ga = raw_adv if 'gate_raw_adv' in mut else adv
        gate = torch.sigmoid((1. if 'gate_sign' in mut else -1.) * lp * ga / p['gate_temp'])
        if 'gate_grad' not in mut:
            gate = gate.detach()
    ratio = torch.exp(lp - old)
    clip = p['clip']
    if p['objective'] == 0:
        s1, s2 = ratio * adv, ratio.clamp(1. - clip, 1. + clip) * adv
        if 'clip_pass' in mut:
            m = s1 + (torch.min(s1, s2) - s1).detach()
        elif 'tie_rule' in mut:
            m = torch.where(s1 < s2, s1, s2.detach())
        else:
            m = torch.min(s1, s2)
        pl = -m * gate
    elif p['objective'] == 1:
        quad = 0. if 'spo_no_quad' in mut else adv.abs() * (ratio - 1.) ** 2 / (2. * clip)
        pl = -(ratio * adv - quad) * gate
    else:
        pos = (adv > 0.) if 'pmpo_sign0' in mut else (adv >= 0.)
        sgn = torch.where(pos, torch.ones_like(adv), -torch.ones_like(adv))
        pl = -(1. if 'no_alpha' in mut else p['pmpo_alpha']) * sgn * lp * torch.tanh(adv).abs() * gate
    aux = sum(kls) if kls else torch.zeros(R, dtype=dtype)
    row_pl, row_ent, row_aux = pl * mask, (ent if 'ent_sign' in mut else -ent) * mask, aux * mask
    loss = row_pl.sum() / count + p['ent_w'] * row_ent.sum() / count
    if kl_on:
        loss = loss + p['kl_w'] * (row_aux.detach() if 'kl_no_grad' in mut else row_aux).sum() / count
    return dict(loss=loss, row_pl=row_pl, row_ent=row_ent, row_aux=row_aux, lp=lp, old=old, ratio=ratio, adv=adv, kls=kls, mask=mask)


def policy_ref(p, dtype=torch.float64, mut=()):
    """p: rows, sizes (tuple), nc, link ('softplus' | 'exp'), logits [R, A] / actions int64 [R, na] / old_lp [R, na] / old_logits [R, A] or None,
    cparams [R, 2 nc] / actions_cont [R, nc] / old_lp_cont [R, nc] / old_cparams [R, nc, 2] or None, adv [R], mask [R] or None, objective 0 / 1 / 2,
    normalize, eps, use_gate, gate_temp, pmpo_alpha, kl_w, reverse_kl, clip, ent_w.
    -> loss [1], dlogits [R, A] (None without discrete actions), dcparams [R, 2 nc] (None without continuous ones), row_pl, row_ent, row_aux [R]."""
    logits = p['logits'].to(dtype).clone().requires_grad_() if p['sizes'] else None
    cparams = p['cparams'].to(dtype).clone().requires_grad_() if p['nc'] else None
    t = policy_terms(p, logits, cparams, dtype, mut)
    leaves = [x for x in (logits, cparams) if x is not None]
    grads = list(torch.autograd.grad(t['loss'], leaves, allow_unused=True)) if t['loss'].requires_grad else [None] * len(leaves)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    res = dict(loss=t['loss'].detach().reshape(1), dlogits=grads.pop(0) if logits is not None else None, dcparams=grads.pop(0) if cparams is not None else None,
               row_pl=t['row_pl'].detach(), row_ent=t['row_ent'].detach(), row_aux=t['row_aux'].detach())
    if 'last_row' in mut:
        res = {k: (x if x is None or k == 'loss' else torch.cat([x[:-1], torch.zeros_like(x[-1:])])) for k, x in res.items()}
    return res


# ------------------------------------------------------------------------------------------------------------------- value loss
def value_ref(p, dtype=torch.float64, mut=()):
    """p: logits [R, bins], returns [R], mask [R] or None, support ([bins + 1] edges, HL-Gauss; [bins] values, two-hot), vmin, vmax, sigma, eps,
    two_hot -> loss [1] = sum_r mask CE_r / max(sum mask, 1) (0 for an all-zero mask) and dv [R, bins]."""
    v = p['logits'].to(dtype).clone().requires_grad_()
    R, bins = v.shape
    sup = p['support'].to(dtype)
    ret = p['returns'].to(dtype)
    mask = torch.ones(R, dtype=dtype) if p['mask'] is None or 'mask_ignored' in mut else p['mask'].to(dtype)
    count = mask.sum() if 'count_unclamped' in mut else mask.sum().clamp(min=1.)
    if p['two_hot']:
        if 'no_clamp' not in mut:
            ret = ret.clamp(sup[0], sup[-1])
        idx = torch.searchsorted(sup, ret, right='side' in mut)
        li = (idx - 1).clamp(min=0)
        ri = (li + 1).clamp(max=bins - 1)
        wl = (sup[ri] - ret) / (sup[ri] - sup[li])
        if 'swap_lr' in mut:
            wl = 1. - wl
        tgt = torch.zeros(R, bins, dtype=dtype)
        tgt.scatter_(1, li[:, None], wl[:, None])
        tgt.scatter_(1, ri[:, None], (1. - wl)[:, None])
    else:
        if 'no_clamp' not in mut:
            ret = ret.clamp(p['vmin'], p['vmax'])
        cdf = torch.special.erf((sup[None, :] - ret[:, None]) / (math.sqrt(2.) * p['sigma']))
        z = cdf[:, -1] - cdf[:, 0]
        tgt = cdf[:, 1:] - cdf[:, :-1]
        if 'no_z' not in mut:
            tgt = tgt / z.clamp(min=p['eps'])[:, None]
    used = bins - 1 if 'last_bin' in mut and bins > 1 else bins
    ls = v[:, :used] - torch.logsumexp(v[:, :used], -1, keepdim=True)
    ce = -(tgt[:, :used] * ls).sum(-1)
    if 'no_psum' in mut:                         # value kept, gradient + (1 - sum target) softmax
        lse = torch.logsumexp(v[:, :used], -1)
        ce = ce + (1. - tgt[:, :used].sum(-1)) * (lse - lse.detach())
    loss = (ce * mask).sum() / count
    dv, = torch.autograd.grad(loss, v)
    if 'last_row' in mut:
        dv = torch.cat([dv[:-1], torch.zeros_like(dv[-1:])])
    return dict(loss=loss.detach().reshape(1), dv=dv)
