"""Plain references of the learner's two actor-critic options (csrc/learn.hip: return_stats_kernel and value_loss_clip_kernel), as
tests/test_gpu_learn_norm_ops.py calls them alone through d4_return_stats and d4_value_loss.  Logical tensors only.  Every function takes a
`dtype` (float64: the reference of the GPU tests; float32: the same code at the kernels' precision, whose distance to float64 is the E32 of
learn_norm_cases.py).  Gradients come from autograd, never from a formula written here; the quantiles from torch.quantile.

`mut` names deliberate mistakes (tests/test_learn_norm_host.py shows that the inputs and the bounds of the GPU tests can see each):
  return statistics
    quantile_nearest          the nearest rank instead of the linear interpolation between two ranks
    quantile_unmasked         the quantiles taken over every return, masked ones included
    no_clamp_stats            mean and variance of the unclamped returns
    var_bessel                the variance with Bessel's correction
    ema_swapped_decay         lerp weight reward_ema_decay instead of 1 - reward_ema_decay
    std_unclamped             sqrt(var) without the clamp at 1e-5
    norm_old_values_skipped   the old values enter the advantage unnormalised
    stats_after_update_order  the advantage formed from the buffers as they were BEFORE the update
    last_row                  the last advantage not written
  clipped value loss
    clip_one_sided            the clamp of values - old from above only
    min_instead_of_max        the smaller of the two losses
    clipped_no_grad           no gradient through the clipped loss
    clamp_grad_passed         the gradient passed through the clamp where it is active
    log_eps_missing           log(q) without the clamp at 1e-20
    values_from_argmax        values = the centre of the largest logit's bin instead of the softmax expectation
    last_row                  the last row not written
    last_bin                  the last bin left out"""
import math

import torch

from learn_ref import err, err_all        # noqa: F401  (one error measure for both families of tests)

STATS_MUTATIONS = ('quantile_nearest', 'quantile_unmasked', 'no_clamp_stats', 'var_bessel', 'ema_swapped_decay', 'std_unclamped', 'norm_old_values_skipped',
                   'stats_after_update_order', 'last_row')
CLIP_MUTATIONS = ('clip_one_sided', 'min_instead_of_max', 'clipped_no_grad', 'clamp_grad_passed', 'log_eps_missing', 'values_from_argmax', 'last_row', 'last_bin')
LOG_EPS = 1e-20
STD_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------- return statistics
def return_stats_ref(p, dtype=torch.float64, mut=()):
    """p: returns [n], old_values [n], mask [n] or None, ema (mean, var), decay, q (lo, hi) as the float32 numbers the kernel is given.
    -> adv [n], ema [2] after the update, stats [4] = lo, hi, mean, var (zeros when nothing is kept)."""
    ret, old = p['returns'].to(dtype), p['old_values'].to(dtype)
    n = ret.numel()
    keep = torch.ones(n, dtype=torch.bool) if p['mask'] is None else p['mask'] != 0
    ema0 = torch.tensor(p['ema'], dtype=torch.float32).to(dtype)            # the buffers are float32
    ema = ema0.clone()
    stats = torch.zeros(4, dtype=dtype)
    if keep.any():
        x = ret[keep]
        q = torch.tensor(p['q'], dtype=torch.float32).to(dtype)
        src = ret if 'quantile_unmasked' in mut else x
        lo, hi = torch.quantile(src, q, interpolation='nearest' if 'quantile_nearest' in mut else 'linear')
        xc = x if 'no_clamp_stats' in mut else x.clamp(lo, hi)
        mean = xc.mean()
        var = xc.var(correction=1 if 'var_bessel' in mut and xc.numel() > 1 else 0)
        w = p['decay'] if 'ema_swapped_decay' in mut else 1. - p['decay']
        w = torch.tensor(w, dtype=torch.float32 if dtype == torch.float32 else torch.float64).to(dtype)
        ema = torch.stack([torch.lerp(ema0[0], mean, w), torch.lerp(ema0[1], var, w)])
        stats = torch.stack([lo, hi, mean, var])
    use = ema0 if 'stats_after_update_order' in mut else ema
    std = use[1].sqrt() if 'std_unclamped' in mut else use[1].clamp(min=STD_EPS).sqrt()
    nold = old if 'norm_old_values_skipped' in mut else (old - use[0]) / std
    adv = (ret - use[0]) / std - nold
    if 'last_row' in mut:
        adv = torch.cat([adv[:-1], torch.zeros_like(adv[-1:])])
    return dict(adv=adv, ema=ema, stats=stats)


def order_statistics(p):
    """The two pairs of neighbouring order statistics the quantiles interpolate between, from the float32 data: [[x_fl, x_ce] for lo, for hi]."""
    keep = torch.ones(p['returns'].numel(), dtype=torch.bool) if p['mask'] is None else p['mask'] != 0
    x = p['returns'][keep].double().sort().values
    out = []
    for q in p['q']:
        pos = float(torch.tensor(q, dtype=torch.float32).double()) * (x.numel() - 1)
        out.append([x[math.floor(pos)].item(), x[math.ceil(pos)].item()])
    return out


# ------------------------------------------------------------------------------------------------------------------- clipped value loss
def encode(x, sup, p, dtype):
    """The value encoder of the returns (tests/learn_ref.py: value_ref), differentiable in x: [R] -> [R, bins]."""
    R = x.numel()
    if p['two_hot']:
        bins = sup.numel()
        x = x.clamp(sup[0], sup[-1])
        idx = torch.searchsorted(sup, x.detach())
        li = (idx - 1).clamp(min=0)
        ri = (li + 1).clamp(max=bins - 1)
        wl = (sup[ri] - x) / (sup[ri] - sup[li])
        enc = torch.zeros(R, bins, dtype=dtype)
        enc = enc.scatter(1, li[:, None], wl[:, None])
        return enc.scatter(1, ri[:, None], (1. - wl)[:, None])
    x = x.clamp(p['vmin'], p['vmax'])
    cdf = torch.special.erf((sup[None, :] - x[:, None]) / (math.sqrt(2.) * p['sigma']))
    z = cdf[:, -1] - cdf[:, 0]
    return (cdf[:, 1:] - cdf[:, :-1]) / z.clamp(min=p['eps'])[:, None]


def centres(sup, two_hot):
    return sup if two_hot else (sup[:-1] + sup[1:]) / 2


def value_clip_terms(p, v, dtype=torch.float64, mut=()):
    """Per-row terms: loss1 (cross entropy), loss2 (clipped), values, and the row loss."""
    sup = p['support'].to(dtype)
    ret, old = p['returns'].to(dtype), p['old_values'].to(dtype)
    R, bins = v.shape
    used = bins - 1 if 'last_bin' in mut and bins > 1 else bins
    tgt = encode(ret, sup, p, dtype)[:, :used]
    ctr = centres(p['support'], p['two_hot']).to(dtype)[:used]           # float32 centres, as the kernel forms them
    ls = v[:, :used] - torch.logsumexp(v[:, :used], -1, keepdim=True)
    loss1 = -(tgt * ls).sum(-1)
    values = ctr[v[:, :used].argmax(-1)] if 'values_from_argmax' in mut else (ls.exp() * ctr).sum(-1)
    diff = values - old
    cl = diff.clamp(max=p['value_clip']) if 'clip_one_sided' in mut else diff.clamp(-p['value_clip'], p['value_clip'])
    if 'clamp_grad_passed' in mut:
        cl = cl.detach() + diff - diff.detach()
    q = encode(old + cl, sup, p, dtype)[:, :used]
    loss2 = -(tgt * (q.log() if 'log_eps_missing' in mut else q.clamp(min=LOG_EPS).log())).sum(-1)
    if 'clipped_no_grad' in mut:
        loss2 = loss2.detach()
    row = torch.minimum(loss1, loss2) if 'min_instead_of_max' in mut else torch.maximum(loss1, loss2)
    return dict(loss1=loss1, loss2=loss2, values=values, row=row, diff=diff)


def value_clip_ref(p, dtype=torch.float64, mut=()):
    """p: value_ref's arguments (tests/learn_ref.py) plus old_values [R] and value_clip -> loss [1], row_loss [R] (masked), dv [R, bins]."""
    v = p['logits'].to(dtype).clone().requires_grad_()
    R = v.shape[0]
    mask = torch.ones(R, dtype=dtype) if p['mask'] is None else p['mask'].to(dtype)
    t = value_clip_terms(p, v, dtype, mut)
    row = t['row'] * mask
    loss = row.sum() / mask.sum().clamp(min=1.)
    dv, = torch.autograd.grad(loss, v)
    row = row.detach()
    if 'last_row' in mut:
        dv, row = torch.cat([dv[:-1], torch.zeros_like(dv[-1:])]), torch.cat([row[:-1], torch.zeros_like(row[-1:])])
    return dict(loss=loss.detach().reshape(1), row_loss=row, dv=dv)
