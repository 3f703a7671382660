"""The yardstick of the bf16 training arithmetic: the ORACLE's own bf16 noise, computed from oracle/restate.py and the fixtures alone.

A bf16-operand computation cannot be compared element-wise with another one: rounding noise re-draws itself under fp32-level differences
(nudging the inputs by one fp32 ulp moves the gradients of a bf16 emulation by ~0.6 %, against 2e-6 for the plain fp32 oracle).  So the
bound for the code under test is an ENVELOPE: how far the oracle itself moves from its fp32 result when its Linears round their operands to
bf16, over four variants of that emulation.  Nothing here reads the code under test.

`bf16_linears(min_out)` replaces `torch.Tensor.__matmul__` (the oracle writes every Linear as `x @ W.t()`; its attention cores are einsums and
stay untouched) by an autograd.Function that rounds both operands to bf16 (round to nearest even) in the forward and dY in the backward, the
products themselves in the tensors' own precision.  The variants: every `@` with a 2-D right operand / only those with at least 16 output
features, each once as is and once with the parameters and inputs multiplied by 1 + 2^-22 (2^-21 for the second)."""
import contextlib

import torch

VARIANTS = ((0, 0.), (16, 0.), (0, 2. ** -22), (16, 2. ** -21))        # (min output features, relative nudge)


def _round(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Bf16Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):                         # w: (in, out) — the oracle's W.t()
        xb, wb = _round(x), _round(w)
        ctx.save_for_backward(xb, wb)
        return torch.matmul(xb, wb)

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        dyb = _round(dy)
        dx = torch.matmul(dyb, wb.t())
        dw = torch.matmul(xb.reshape(-1, xb.shape[-1]).t(), dyb.reshape(-1, dyb.shape[-1]))
        return dx, dw


@contextlib.contextmanager
def bf16_linears(min_out=0):
    orig = torch.Tensor.__matmul__

    def matmul(a, b):
        if torch.is_tensor(b) and b.ndim == 2 and a.ndim >= 2 and a.is_floating_point() and b.shape[1] >= min_out:
            return _Bf16Linear.apply(a, b)
        return orig(a, b)

    torch.Tensor.__matmul__ = matmul
    try:
        yield
    finally:
        torch.Tensor.__matmul__ = orig


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def scaled_max(a, b):
    """max |a - b| / max |b|: the metric of the fp32 block tests (tests/test_gpu_backward.py `close`)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-6))


def run_variants(run):
    """run(nudge) -> dict name -> tensor (outputs, losses, gradients), called inside each variant's emulation.  Returns the list of the
    four variants' dicts."""
    outs = []
    for min_out, nudge in VARIANTS:
        with bf16_linears(min_out):
            outs.append({k: v.detach().clone() for k, v in run(nudge).items()})
    return outs


def envelope(outs, ref, metric):
    """E_max[k] = max over the variants of metric(variant[k], ref[k])."""
    return {k: max(metric(o[k], ref[k]) for o in outs) for k in ref}


def global_rel_l2(d, ref, keys):
    cat = lambda x: torch.cat([x[k].detach().double().cpu().flatten() for k in keys])
    return rel_l2(cat(d), cat(ref))


# ------------------------------------------------------------------------------------------------ the model fixtures
def _nudged(W, keys, nudge, dtype=None):
    out = {}
    for k, v in W.items():
        if k in keys:
            v = v.clone() if dtype is None else v.to(dtype)
            out[k] = (v * (1. + nudge) if nudge else v).detach().requires_grad_()
        else:
            out[k] = v
    return out


def train_fixture(name='shortcut'):
    """train.npz: (run, ref) — run(nudge) = the oracle's flow + shortcut losses and the gradients of their sum, ref = the fixture's."""
    from oracle import restate
    from util import golden_oracle, load_golden, t
    g = load_golden('train.npz')
    cfg, W = golden_oracle('weights_train.npz')
    keys = [k[len(name) + 6:] for k in g if k.startswith(name + '_grad/')]
    ref = {'loss/flow': t(g[name + '_flow_loss']), 'loss/shortcut': t(g[name + '_shortcut_loss'])}
    ref.update({'grad/' + k: t(g[f'{name}_grad/{k}']) for k in keys})

    def run(nudge):
        Wg = _nudged(W, keys, nudge)
        lat = t(g['latents']) * (1. + nudge)
        fl, sl = restate.dynamics_flow_losses(cfg, Wg, lat, t(g[name + '_noise']), t(g[name + '_signal_levels']), t(g[name + '_step_sizes_log2']),
                                              name == 'shortcut', actions=t(g['actions']))
        (fl + sl).backward()
        out = {'loss/flow': fl, 'loss/shortcut': sl}
        out.update({'grad/' + k: Wg[k].grad for k in keys})
        return out
    return run, ref


def train_agent_fixture():
    """train_agent.npz: the whole training forward (rewards, terminals, two action types): every loss term and the gradients of the total."""
    from oracle import restate
    from util import golden_oracle, load_golden, t
    g = load_golden('train_agent.npz')
    cfg, W = golden_oracle('weights_train_agent.npz')
    keys = [k[5:] for k in g if k.startswith('grad/')]
    terms = ('flow', 'shortcut', 'rewards', 'terminals', 'discrete_actions')
    ref = {'loss/' + n: t(g[n + '_loss']) for n in terms}
    ref['loss/total'] = t(g['total'])
    ref.update({'grad/' + k: t(g['grad/' + k]) for k in keys})

    def run(nudge):
        Wg = _nudged(W, keys, nudge)
        lat = t(g['latents']) * (1. + nudge)
        out_ = restate.dynamics_training_losses(cfg, Wg, lat, t(g['noise']), t(g['signal_levels']), t(g['step_sizes_log2']), True,
                                                actions=t(g['actions']), rewards=t(g['rewards']), terminals=t(g['terminals']))
        out_['total'].backward()
        out = {'loss/' + n: out_[n] for n in terms}
        out['loss/total'] = out_['total']
        out.update({'grad/' + k: Wg[k].grad for k in keys})
        return out
    return run, ref


def model_envelope(run, ref):
    """(E_max per gradient tensor, G_max, L_max per loss term, the variants' outputs) for a model fixture."""
    outs = run_variants(run)
    gkeys = [k for k in ref if k.startswith('grad/')]
    lkeys = [k for k in ref if k.startswith('loss/')]
    E = {k: max(rel_l2(o[k], ref[k]) for o in outs) for k in gkeys}
    G = max(global_rel_l2(o, ref, gkeys) for o in outs)
    L = {k: max(float((o[k].double() - ref[k].double()).abs().max()) for o in outs) for k in lkeys}
    return E, G, L, outs


def check_model(got, ref, E, G, L, report=None):
    """The issue's table: every gradient tensor <= 3 E_max + 1e-3 (relative l2; 1e-3 = the fp32 path's gradient tolerance), all gradients
    concatenated <= 1.25 G_max, every loss term <= 3 L_max + 1e-5 |fixture| (1e-5 = the fp32 tests' loss tolerance).  Returns the failures;
    `report`, when a list, receives one line per quantity (value, bound, ratio)."""
    bad = []
    gkeys = [k for k in ref if k.startswith('grad/')]
    for k in gkeys:
        d, bound = rel_l2(got[k], ref[k]), 3. * E[k] + 1e-3
        if report is not None:
            report.append(f'{k}: rel l2 {d:.3e}  E_max {E[k]:.3e}  bound {bound:.3e}  ratio-to-E_max {d / max(E[k], 1e-30):.2f}')
        if not d <= bound:
            bad.append((k, d, bound))
    d, bound = global_rel_l2(got, ref, gkeys), 1.25 * G
    if report is not None:
        report.append(f'all gradients: rel l2 {d:.3e}  G_max {G:.3e}  bound {bound:.3e}  ratio-to-G_max {d / G:.3f}')
    if not d <= bound:
        bad.append(('all gradients', d, bound))
    for k in L:
        d = float((got[k].detach().double().cpu() - ref[k].double()).abs().max())
        bound = 3. * L[k] + 1e-5 * float(ref[k].double().abs().max())
        if report is not None:
            report.append(f'{k}: |diff| {d:.3e}  L_max {L[k]:.3e}  bound {bound:.3e}  at {float(ref[k].double().abs().max()):.3e}')
        if not d <= bound:
            bad.append((k, d, bound))
    return bad
