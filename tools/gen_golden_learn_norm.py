"""Generate tests/golden/learn_norm.npz from the REFERENCE itself (build container only; needs the reference checkout, see oracle/ref_import.py):

    python tools/gen_golden_learn_norm.py

learn_from_experience with keep_reward_ema_stats=True and clip_values=True (dreamer4.py:5985-6015, 6283-6291), called TWICE in a row on
one small experience so that the EMA pair is carried from the first call into the second.  The reference reads both flags, value_clip and
reward_ema_decay at call time and always registers the buffers, so they are set on a model built by oracle/ref_harness.py.

Two models, both from weights that are fixtures already (no new weights file):
    hl      weights_learn_full.npz (HL-Gauss value head) on the experience of learn_full.npz  — also run with only_learn_policy_value_heads=False
    symexp  weights_symexp.npz (two-hot value head) on the experience of symexp.npz, two trajectories cut short
The stored behaviour values are moved off the current value head's predictions (an off-policy experience) and the rewards scaled, so that in the
reference's own run both branches of the maximum and both sides of the clamp occur; the script asserts that and records, per row, the branch
(clipped loss larger) and the side of the clamp (-1 / 0 / +1), taken from the reference's own tensors through hooks on its value encoder.
Per model and objective (ppo, pmpo), per call: both losses, the head gradients (small ones whole, large ones as norm + every 97th element), and
the EMA pair after the call; once: the GAE returns.  Data only."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle.ref_harness import build_reference_model          # noqa: E402
from oracle.ref_import import load_reference                  # noqa: E402
from oracle.restate import Config                             # noqa: E402
from util import golden_config_kwargs, load_golden            # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'learn_norm.npz')
HEADS = ('policy_head', 'value_head', 'action_embedder.discrete_action_unembed')
# model -> weights, experience file and prefix, step size, value_clip, reward scale, spread of the behaviour values around the predictions
MODELS = dict(hl=('weights_learn_full.npz', 'learn_full.npz', 'exp_', 4, 0.3, 0.6, 1.0),
              symexp=('weights_symexp.npz', 'symexp.npz', 'cached_', 16, 0.3, 0.02, 1.0))
DECAY = 0.9          # (the default 0.998 moves the pair by 0.2 % a call: a carry that small would hide in the tolerances)


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def reference_model(weights):
    kw = golden_config_kwargs(weights)
    kw = {k: (str(v) if isinstance(v, np.str_) else v) for k, v in kw.items()}
    m = build_reference_model(Config(**kw), seed=0)
    W = {k: torch.from_numpy(v) for k, v in load_golden(weights).items() if not k.startswith(('cfg_', 'meta_'))}
    res = m.load_state_dict(W, strict=False)
    assert not res.unexpected_keys and all(dict(m.state_dict())[k].numel() == 0 for k in res.missing_keys), res
    return m


def experience(D4, g, p, step_size, name, reward_scale, spread):
    t = lambda k: torch.from_numpy(g[p + k])
    lens, terminals = t('lens').clone(), t('terminals').clone()
    if name == 'symexp':                     # the stored rollout ran to the end everywhere: cut two trajectories short
        lens, terminals = torch.tensor([5, 3, 4]), torch.tensor([False, True, True])
    gen = torch.Generator().manual_seed(4242)
    values = t('values') + spread * torch.randn(t('values').shape, generator=gen)
    return D4.Experience(latents=t('latents'), agent_embed=t('agent_embed'), rewards=t('rewards') * reward_scale, values=values,
                         log_probs=D4.Actions(t('log_probs'), None), actions=D4.Actions(t('actions'), None), lens=lens, terminals=terminals,
                         is_truncated=~terminals, old_action_unembeds=D4.Actions(t('unembeds'), None), step_size=step_size)


def grads_into(out, tag, m):
    for k, p in m.named_parameters():
        if k.startswith(HEADS) and p.numel() > 0 and p.grad is not None:
            if p.ndim == 1 or 'unembed' in k or p.numel() <= 1024:
                out[f'{tag}_grad/{k}'] = npy(p.grad)
            else:
                out[f'{tag}_gnorm/{k}'] = npy(p.grad.norm())
                out[f'{tag}_gsample/{k}'] = npy(p.grad.flatten()[::97])


def main():
    D4 = load_reference()
    out = {}
    for name, (weights, expf, prefix, step, clip, rscale, spread) in MODELS.items():
        g = load_golden(expf)
        e = experience(D4, g, prefix, step, name, rscale, spread)
        for k in ('latents', 'agent_embed', 'rewards', 'values', 'lens', 'terminals'):
            out[f'{name}_exp_{k}'] = npy(getattr(e, k))
        out[f'{name}_exp_log_probs'], out[f'{name}_exp_actions'], out[f'{name}_exp_unembeds'] = npy(e.log_probs.discrete), npy(e.actions.discrete), npy(e.old_action_unembeds.discrete)
        out[f'{name}_step_size'], out[f'{name}_value_clip'], out[f'{name}_decay'] = np.array(step), np.array(clip), np.array(DECAY)
        out[f'{name}_weights'], out[f'{name}_experience'] = np.array(weights), np.array(expf)
        for obj in ('ppo', 'pmpo'):
            for full in ((False, True) if name == 'hl' and obj == 'ppo' else (False,)):
                m = reference_model(weights)
                m.keep_reward_ema_stats, m.clip_values, m.value_clip, m.reward_ema_decay = True, True, clip, DECAY
                seen = []                    # inputs of the value encoder: the returns first, the clipped values second
                hook = m.value_encoder.register_forward_hook(lambda mod, args, res: seen.append(args[0].detach().clone()))
                tag0 = f"{name}_{obj}{'_full' if full else ''}"
                for call in (1, 2):
                    m.zero_grad()
                    del seen[:]
                    pl, vl = m.learn_from_experience(e, objective=obj, only_learn_policy_value_heads=not full)
                    tag = f'{tag0}_call{call}'
                    out[f'{tag}_policy_loss'], out[f'{tag}_value_loss'] = npy(pl), npy(vl)
                    out[f'{tag}_ema'] = np.array([float(m.ema_returns_mean), float(m.ema_returns_var)], dtype=np.float32)
                    if full:
                        pl.backward(retain_graph=True)
                        trunk = {k: p.grad for k, p in m.named_parameters() if p.grad is not None and p.numel() > 0 and not k.startswith(HEADS) and float(p.grad.abs().max()) > 0}
                        for k, gr in trunk.items():
                            out[f'{tag}_pgnorm/{k}'] = npy(gr.norm())
                        m.zero_grad()
                        vl.backward()
                        for k, p in m.named_parameters():
                            if p.grad is not None and p.numel() > 0 and float(p.grad.abs().max()) > 0:
                                out[f'{tag}_vgnorm/{k}'] = npy(p.grad.norm())
                        print(tag, 'trunk gradients', len(trunk))
                    else:
                        pl.backward(); vl.backward()
                        grads_into(out, tag, m)
                    returns, clipped = seen[0], seen[1]
                    print(tag, 'policy', float(pl), 'value', float(vl), 'ema', out[f'{tag}_ema'])
                hook.remove()
                if obj == 'ppo' and not full:
                    # per row, from the reference's own tensors: the side of the clamp, and the branch of the maximum recomputed from its encoder
                    T = returns.shape[1]
                    old = e.values.masked_fill(~(torch.arange(T)[None] < e.lens[:, None]), 0.)
                    side = torch.sign(((clipped - old) / clip).round()) * (((clipped - old).abs() - clip).abs() < 1e-6)
                    with torch.no_grad():
                        vb = m.value_head(e.agent_embed)
                        vb = vb[..., 0, :] if vb.ndim == 4 else vb
                        rb, cb = m.value_encoder(returns), m.value_encoder(clipped)
                        l1 = -(rb * vb.log_softmax(-1)).sum(-1)
                        l2 = -(rb * cb.clamp(min=1e-20).log()).sum(-1)
                    mask = torch.arange(T)[None] < (e.lens - (~e.terminals).long())[:, None]
                    out[f'{name}_returns'], out[f'{name}_clipped'], out[f'{name}_side'], out[f'{name}_branch'], out[f'{name}_mask'] = \
                        npy(returns), npy(clipped), npy(side), npy(l2 > l1), npy(mask)
                    print(name, 'side', side[mask].tolist(), 'branch', (l2 > l1)[mask].tolist(), 'l1', l1[mask].tolist(), 'l2', l2[mask].tolist())
                    assert {-1., 0., 1.} <= set(side[mask].tolist()) or {-1., 1.} <= set(side[mask].tolist()), 'both sides of the clamp must occur among the learnable rows'
                    assert (l2 > l1)[mask].any() and (l1 > l2)[mask].any(), 'both branches of the maximum must occur among the learnable rows'
    np.savez(OUT, **out, meta_reference=np.array('lucidrains/dreamer4 dreamer4/dreamer4.py imported unmodified through oracle/shim'))
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
