"""Generate the fixtures of the VideoTokenizer training forward from the REFERENCE itself (build container only, like oracle/gen_golden.py):

    python tools/gen_tok_train_golden.py          # needs the reference checkout (oracle/ref_import.py); writes tests/golden/

  tok_train.npz       + weights_tok_train.npz        dim 32, 6 latents x 8, patch 4, 16 x 24 x 3 (24 patches + 6 latents = 30 tokens per frame),
                                                     depths 2 / 2, time block every 2, 2 heads x 64, decoder_flow_steps 2; video (2, 3, 3, 16, 24)
  tok_train_wide.npz  + weights_tok_train_wide.npz   32 x 40 x 1, 5 latents x 4 (80 patches + 5 latents = 85 tokens: the smallest frame past 64),
                                                     depths 2 / 2, 1 head; video (1, 1, 2, 32, 40)

The reference's dreamer4.py is imported unmodified through oracle/ref_import.py (the third-party stand-ins of oracle/shim); tokenizers are built as
oracle/gen_golden.py::_reference_tokenizer builds them (lpips_loss_weight = 0.).  The reference's own random draws are recorded as they are made
(torch.bernoulli, randint, randn_like patched to record).  Two things are shaped rather than merely recorded, and both are stored as data:
  * the Bernoulli patch mask: frame 0 of every clip is left unmasked and the first half of frame 1's patches is masked on top of the draw (image
    batches: clip 0 unmasked, half of clip 1 masked), so that `mask_token` gets a gradient and both kinds of frame occur;
  * the seed of a case: the first one at which the drawn `time_indices` are not all 0.
oracle/shim/einx.py has no `where`; the one pattern the masking uses ('..., d, ... d', dreamer4.py:4344) is supplied here as torch.where.

Cases of the narrow fixture (all in train() mode): `train` (masking), `train2` (the next call: carries the normaliser state), `nonorm`
(use_loss_normalization False), `xspace` (decoder_v_space_loss False), `image` (a (2, 3, 16, 24) batch), `latents` (return_latents with a given
patch_mask).  Per case: video, the three draws, recon, total, latents, recon_video, the normaliser state before and after, and the gradient of
total with respect to EVERY parameter except decoder.transformer.final_special_* (whose output the decoder never reads) and the encoder's
final_special_cross_attn.fn.to_learned_value_residual_mix.0.* (the reference constructs that projection but calls the special-token cross attention
without residual values, so nothing reads it): those are asserted None or zero here, every other gradient is asserted non-zero
(but for the image case: over a single frame the belief projection cancels a time layer's attention output, so every gradient inside that
block is float32 rounding noise around zero; asserted below 1e-6 of the case's largest gradient and not recorded).

A committed file stays under 1 MiB: a fixture whose arrays exceed that is written as NAME.npz, NAME.p1.npz, ... (tests/tok_train_cases.py
`load_parts` merges them)."""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness                                     # noqa: E402,F401  (the reference harness: import path set-up)
from oracle.gen_golden import META, _reference_tokenizer, npy      # noqa: E402
from oracle.ref_import import load_reference                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
PART_BYTES = 900 * 1024
UNREAD = 'decoder.transformer.final_special_'
UNUSED = 'final_special_cross_attn.fn.to_learned_value_residual_mix.'     # the cross attention is called without residual values (dreamer4.py:3227-3234)


def time_attention(tok, k):
    """k names a parameter of a time layer's attention block (layers.N.2.fn.* with N a time layer)"""
    if '.layers.' not in k or '.2.fn.' not in k:
        return False
    return bool(tok.encoder_transformer.is_time[int(k.split('.layers.')[1].split('.')[0])])


def unread(k):
    return k.startswith(UNREAD) or UNUSED in k

CFG_NARROW = dict(dim=32, dim_latent=8, patch_size=4, image_height=16, image_width=24, num_latent_tokens=6, encoder_depth=2, decoder_depth=2,
                  time_block_every=2, attn_heads=2, attn_dim_head=64, channels=3, decoder_flow_steps=2)
CFG_WIDE = dict(dim=32, dim_latent=4, patch_size=4, image_height=32, image_width=40, num_latent_tokens=5, encoder_depth=2, decoder_depth=2,
                time_block_every=2, attn_heads=1, attn_dim_head=64, channels=1, decoder_flow_steps=2)


def save_parts(name, arrays):
    """np.savez in parts of at most PART_BYTES of array data: NAME.npz, NAME.p1.npz, ...; stale parts of an earlier run are removed."""
    stem = name[:-4]
    for f in os.listdir(OUT):
        if f.startswith(stem + '.p') and f.endswith('.npz'):
            os.remove(os.path.join(OUT, f))
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        v = np.asarray(v)
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur); cur, size = {}, 0
        cur[k] = v; size += v.nbytes + 256
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(OUT, name if i == 0 else f'{stem}.p{i}.npz')
        np.savez(path, **part)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    return len(parts)


@contextlib.contextmanager
def recorded_draws(D4, rec):
    import einx
    saved = (torch.bernoulli, D4.randint, D4.randn_like, einx.where)

    def bernoulli(p, *a, **k):
        r = saved[0](p, *a, **k)
        flat = r.flatten(2)                                            # (b, t, patches)
        half = (flat.shape[-1] + 1) // 2
        if r.shape[1] >= 2:
            flat[:, 0] = 0.; flat[:, 1, :half] = 1.
        else:
            flat[0] = 0.; flat[1:, :, :half] = 1.
        rec['patch_mask'] = (r == 1.).clone()
        return r

    def randint(*a, **k):
        r = saved[1](*a, **k); rec['time_indices'] = r.clone(); return r

    def randn_like(*a, **k):
        r = saved[2](*a, **k); rec['noise'] = r.clone(); return r

    torch.bernoulli, D4.randint, D4.randn_like = bernoulli, randint, randn_like
    einx.where = lambda pattern, cond, x, y: torch.where(cond[..., None], x, y) if pattern == '..., d, ... d' else saved[3](pattern, cond, x, y)
    try:
        yield
    finally:
        torch.bernoulli, D4.randint, D4.randn_like, einx.where = saved


def norm_state(tok):
    n = getattr(tok, 'recon_loss_normalizer', None)
    return n.exp_avg_sq.detach().clone() if n is not None else torch.ones(1)


def run_case(D4, tok, out, name, x, seed0, **fw):
    """One training forward + backward under recorded draws; the seed is the first from seed0 on whose time_indices are not all 0."""
    lat = {}
    hook = tok.encoded_to_latents.register_forward_hook(lambda m, a, o: lat.__setitem__('latents', o.detach().tanh()))
    before = norm_state(tok)
    try:
        for seed in range(seed0, seed0 + 64):
            rec = {}
            with torch.no_grad():
                if getattr(tok, 'recon_loss_normalizer', None) is not None:
                    tok.recon_loss_normalizer.exp_avg_sq.copy_(before)
            tok.zero_grad()
            torch.manual_seed(seed)
            with recorded_draws(D4, rec):
                total, (losses, recon_video) = tok(x, return_intermediates=True, **fw)
            if bool(rec['time_indices'].any()):
                break
        else:
            raise AssertionError('no seed with a non-zero time index')
    finally:
        hook.remove()
    total.backward()
    assert bool(rec['time_indices'].any()), 'recorded time_indices are all 0'
    pm = rec['patch_mask'].flatten(2)
    if pm.shape[1] >= 2:
        assert bool((~pm.any(-1)).any(1).all()) and bool((pm.float().mean(-1) >= 0.5).any(1).all()), 'patch mask: an unmasked and a half-masked frame per clip'
    for k in ('patch_mask', 'time_indices', 'noise'):
        out[f'{name}_{k}'] = npy(rec[k])
    out[f'{name}_video'], out[f'{name}_seed'] = npy(x), np.array(seed)
    out[f'{name}_recon'], out[f'{name}_total'], out[f'{name}_latents'], out[f'{name}_recon_video'] = npy(losses.recon.reshape(())), npy(total.reshape(())), npy(lat['latents']), npy(recon_video)
    for f in losses._fields:
        if f != 'recon':
            assert float(getattr(losses, f)) == 0., f
    out[f'{name}_norm_before'], out[f'{name}_norm_after'] = npy(before), npy(norm_state(tok))
    ng, noise_keys = 0, []
    for k, p in tok.named_parameters():
        if unread(k):
            assert p.grad is None or float(p.grad.abs().max()) == 0., k
            continue
        assert p.grad is not None, f'{name}: no gradient on {k}'
        if x.ndim == 4 and time_attention(tok, k):
            # one frame: the belief projection of a time layer removes the value direction from an attention over a single key, so the block's output is
            # identically zero and every gradient in it is rounding noise of the float32 evaluation.  Asserted to be that, and not recorded.
            noise_keys.append(k)
            continue
        assert float(p.grad.abs().max()) > 0., f'{name}: zero gradient on {k}'
        out[f'{name}_grad/{k}'] = npy(p.grad); ng += 1
    gmax = max(float(p.grad.abs().max()) for p in tok.parameters() if p.grad is not None)
    for k in noise_keys:
        assert float(tok.get_parameter(k).grad.abs().max()) <= 1e-6 * gmax, k
    print(name, 'seed', seed, 'recon', float(losses.recon), 'total', float(total), 'time_indices', rec['time_indices'].tolist(),
          'masked', rec['patch_mask'].flatten(2).sum(-1).tolist(), 'grads', ng, 'norm', norm_state(tok).tolist())


def weights_of(tok):
    return {k: v.detach().clone().float() for k, v in tok.state_dict().items() if 'loss_normalizer' not in k}


def save_weights(name, W, cfgd):
    return save_parts(name, {**{k: npy(v) for k, v in W.items() if v.numel() > 0}, **{'meta_' + k: np.array(v) for k, v in META.items()},
                             **{'cfg_' + k: np.array(v) for k, v in cfgd.items()}})


def gen_narrow(D4):
    tok, g = _reference_tokenizer(D4, CFG_NARROW, 81)
    tok.train()
    with torch.no_grad():
        tok.mask_token.mul_(30.)                                       # init std 1e-2: make the mask token matter, like the latent tokens
    nw = save_weights('weights_tok_train.npz', weights_of(tok), CFG_NARROW)
    video = torch.rand(2, 3, 3, 16, 24, generator=g)
    image = torch.rand(2, 3, 16, 24, generator=g)
    out = {}
    run_case(D4, tok, out, 'train', video, 100)
    run_case(D4, tok, out, 'train2', video, 200)
    tok.use_loss_normalization = False
    run_case(D4, tok, out, 'nonorm', video, 300)
    tok.use_loss_normalization, tok.decoder_v_space_loss = True, False
    run_case(D4, tok, out, 'xspace', video, 400)
    tok.decoder_v_space_loss = True
    run_case(D4, tok, out, 'image', image, 500)
    pm = torch.rand(2, 3, 4, 6, generator=g) < 0.4
    pm[:, 0] = False
    with recorded_draws(D4, {}), torch.no_grad():
        lat = tok(video, return_latents=True, patch_mask=pm)
    out['latents_video'], out['latents_patch_mask'], out['latents_latents'] = npy(video), npy(pm), npy(lat)
    n = save_parts('tok_train.npz', {**out, **{'meta_' + k: np.array(v) for k, v in META.items()}})
    print('narrow: weights in', nw, 'file(s), fixture in', n)


def gen_wide(D4):
    tok, g = _reference_tokenizer(D4, CFG_WIDE, 83)
    tok.train()
    with torch.no_grad():
        tok.mask_token.mul_(30.)
    nw = save_weights('weights_tok_train_wide.npz', weights_of(tok), CFG_WIDE)
    out = {}
    run_case(D4, tok, out, 'train', torch.rand(1, 1, 2, 32, 40, generator=g), 600)
    n = save_parts('tok_train_wide.npz', {**out, **{'meta_' + k: np.array(v) for k, v in META.items()}})
    print('wide: weights in', nw, 'file(s), fixture in', n)


if __name__ == '__main__':
    D4 = load_reference()
    gen_narrow(D4)
    gen_wide(D4)
