"""Plain-torch restatements of the tokenizer's latent regularisers: the two operators of csrc/tok_reg.hip written out in real arithmetic with
their gradients (`sigreg_ref`, `latent_ortho_ref`), the same two losses as differentiable torch expressions (`sigreg_loss`, `ortho_loss`), and
the three-term extension of the training forward of tests/tok_train_ref.py (`training_forward`).

Every operator restatement takes `dtype`: float64 is the yardstick; float32 is the same formula in the kernels' number format with the long sums added
in the kernels' own order (tests/tok_reg_cases.py derives the tolerance from the two): the characteristic function's sum over the rows in blocks of 64
rows, then the blocks; a Gram row's terms one after the other; sums over the rows of a frame (column means, the frame's loss) per wave over every fourth
row, then the four waves."""
import numpy as np
import torch

import tok_train_ref as T
from oracle import restate

NORM_EPS = 1e-12                                           # F.normalize


def seq_sum(x, dim, dtype):
    """sum over `dim`; in float32 the terms are added in order"""
    if dtype == torch.float64:
        return x.sum(dim=dim)
    return torch.from_numpy(np.asarray(np.take(np.cumsum(x.numpy().astype(np.float32), axis=dim, dtype=np.float32), -1, axis=dim)).copy())


def blocked_sum(x, dim, dtype, block=64):
    """sum over `dim` as d4_sigreg_fwd_bwd adds it: the terms of a block of `block` in order, then the blocks in order"""
    if dtype == torch.float64:
        return x.sum(dim=dim)
    parts = [seq_sum(c, dim, dtype) for c in x.split(block, dim=dim)]
    return seq_sum(torch.stack(parts, dim=dim), dim, dtype)


def wave_rows_sum(x, dim, dtype):
    """sum over the rows of a frame as d4_latent_ortho_fwd_bwd adds it: wave w adds rows w, w + 4, ... in order, then ((w0 + w1) + w2) + w3"""
    if dtype == torch.float64:
        return x.sum(dim=dim)
    idx = torch.arange(x.shape[dim])
    w = [seq_sum(x.index_select(dim, idx[k::4]), dim, dtype) if len(idx[k::4]) else torch.zeros_like(x.select(dim, 0)) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def unit_rows(v):
    return v / v.norm(dim=-1, keepdim=True).clamp(min=NORM_EPS)


def trapezoid_weights(t):
    w = torch.zeros_like(t)
    h = (t[1:] - t[:-1]) / 2
    w[:-1] += h
    w[1:] += h
    return w


# ----------------------------------------------------------------------------- the operators, with their gradients written out
def sigreg_ref(x, projs, lo, hi, num_knots, *, dtype=torch.float64):
    """sigreg(x) without a mask (dreamer4.py:728-767), x (K, ..., d), projs (M, d) the raw draw -> (loss, d loss / d x).  Real arithmetic:
    ecf = C + iS with C, S the means over the rows of cos / sin(t p); |ecf - phi|^2 = (C - phi)^2 + S^2."""
    x, v = x.to(dtype), projs.to(dtype)
    K, d, M = x.shape[0], x.shape[-1], v.shape[0]
    xr = x.reshape(K, -1, d)
    N = xr.shape[1]
    u = unit_rows(v)
    t = torch.linspace(lo, hi, num_knots, dtype=dtype)
    phi = (-0.5 * t.square()).exp()
    p = torch.einsum('knd,md->knm', xr, u)
    ang = p[..., None] * t                                                     # K N M T: test sizes only
    c, s = ang.cos(), ang.sin()
    C, S = blocked_sum(c, 1, dtype) / N, blocked_sum(s, 1, dtype) / N          # K M T
    err = ((C - phi).square() + S.square()) * phi
    loss = torch.trapz(err, t, dim=-1).mean()
    g = (2. / (N * K * M)) * trapezoid_weights(t) * phi * t                    # T
    dp = (c * (g * S)[:, None] - s * (g * (C - phi))[:, None]).sum(dim=-1)     # K N M
    return loss, torch.einsum('knm,md->knd', dp, u).reshape(x.shape)


def latent_ortho_ref(x, *, dtype=torch.float64):
    """orthogonal_loss(x) (dreamer4.py:389-402), x (..., n, d) -> (loss, d loss / d x)"""
    x = x.to(dtype)
    n, d = x.shape[-2:]
    xf = x.reshape(-1, n, d)
    F = xf.shape[0]
    if n == 1:
        return x.new_zeros(()), torch.zeros_like(x)
    xc = xf - wave_rows_sum(xf, 1, dtype)[:, None] / n
    norm = xc.norm(dim=-1, keepdim=True)
    r = norm.clamp(min=NORM_EPS)
    y = xc / r
    G = y @ y.transpose(-1, -2)
    G = G.masked_fill(torch.eye(n, dtype=torch.bool), 0.)
    loss = seq_sum(wave_rows_sum(seq_sum(G.square(), 2, dtype), 1, dtype), 0, dtype) / F     # a row's terms in order, the rows per wave, the frames in order
    dy = (4. / F) * seq_sum(G[..., None] * y[:, None], 2, dtype)               # F n d = sum_j G_ij y_j
    dxc = torch.where(norm > NORM_EPS, (dy - y * (y * dy).sum(dim=-1, keepdim=True)) / r, dy / r)
    dx = dxc - wave_rows_sum(dxc, 1, dtype)[:, None] / n
    return loss, dx.reshape(x.shape)


# ----------------------------------------------------------------------------- the same losses under autograd
def sigreg_loss(x, projs, lo=-5., hi=5., num_knots=17):
    xr = x.reshape(x.shape[0], -1, x.shape[-1])
    t = torch.linspace(lo, hi, num_knots, dtype=x.dtype)
    phi = (-0.5 * t.square()).exp()
    ang = torch.einsum('knd,md->knm', xr, unit_rows(projs.to(x.dtype)))[..., None] * t
    C, S = ang.cos().mean(dim=1), ang.sin().mean(dim=1)
    return torch.trapz(((C - phi).square() + S.square()) * phi, t, dim=-1).mean()


def ortho_loss(x):
    n = x.shape[-2]
    if n == 1:
        return x.new_zeros(())
    y = unit_rows(x - x.mean(dim=-2, keepdim=True))
    G = (y @ y.transpose(-1, -2)).masked_fill(torch.eye(n, dtype=torch.bool), 0.)
    return G.square().sum(dim=(-1, -2)).mean()


# ----------------------------------------------------------------------------- the whole training forward with the three terms
TERMS = ('recon', 'latent_ortho', 'latent_consistency', 'latent_sigreg')
ENCODER_KEYS = ('latent_tokens', 'mask_token', 'patch_to_tokens.', 'encoder_transformer.', 'encoded_to_latents.')      # dreamer4.py:4060-4067


def encoder_pre_latents(tc, W, rows, patch_mask=None):
    """tok_train_ref.encoder_latents from patch rows (b, t, nh, nw, p1 p2 c), up to encoded_to_latents: the latents before the tanh"""
    b, t = rows.shape[:2]
    x = rows @ W['patch_to_tokens.1.weight'].t() + W['patch_to_tokens.1.bias']
    x = restate.layernorm(x, W['patch_to_tokens.2.weight'], 0.)
    if patch_mask is not None:
        x = torch.where(patch_mask[..., None], W['mask_token'], x)
    x = x.reshape(b, t, -1, tc.dim)
    tokens = torch.cat((x, W['latent_tokens'].expand(b, t, -1, -1)), dim=2)
    tokens, _ = restate.transformer(tc.encoder_trunk(), W, tokens, None, pre='encoder_transformer.', num_special=tc.num_latent_tokens)
    return tokens[:, :, x.shape[2]:] @ W['encoded_to_latents.weight'].t()


def normalize(loss, state, update):
    """LossNormalizer.forward (dreamer4.py:645-669); state None: no normalisation"""
    if state is None:
        return loss
    rms = state.sqrt()
    if update:
        state.lerp_(loss.detach().reshape(1).square().to(state.dtype), 1. - 0.95)
    return loss / rms.clamp(min=1e-6).reshape(())


def training_forward(tc, W, video, draws, *, weights, sigreg_kwargs, v_space=True, norm_states=None, update=True):
    """VideoTokenizer.forward (dreamer4.py:4239-4603) with the latent SIGReg, orthogonality and consistency terms, in the dtype of `video` and W.
    draws: tok_train_ref's plus sigreg_projs (num_slices, dim_latent).  weights: dict(latent_sigreg=, latent_ortho=, latent_consistency=).
    norm_states: None or dict(term -> running mean square (1,)), updated in place when `update`.  -> dict(the four terms, total, latents, recon_video)"""
    pm = draws.get('patch_mask')
    pre = encoder_pre_latents(tc, W, T.patch_rows(video, tc.patch_size), pm)
    out = dict(latent_sigreg=sigreg_loss(pre, draws['sigreg_projs'], *sigreg_kwargs.get('domain', (-5., 5.)), sigreg_kwargs.get('num_knots', 17)))
    latents = pre.tanh()
    ti, noise = draws['time_indices'], draws['noise'].to(video.dtype)
    tt = (ti.to(video.dtype) / tc.decoder_flow_steps)[:, None, None, None, None]
    noised = torch.lerp(noise, video, tt)
    recon_video = T.rows_to_video(T.decoder_rows(tc, W, latents, noised, ti), tc.channels, tc.patch_size)
    frozen = {k: (v.detach() if k.startswith(ENCODER_KEYS) else v) for k, v in W.items()}
    recon_latents = encoder_pre_latents(tc, frozen, T.patch_rows(recon_video, tc.patch_size), pm).tanh()
    out['latent_consistency'] = (recon_latents - latents.detach()).pow(2).mean()
    if v_space:
        pred, target = (recon_video - noised) / (1. - tt), video - noise
    else:
        pred, target = recon_video, video
    out['recon'] = (pred - target).pow(2).mean()
    out['latent_ortho'] = ortho_loss(latents)
    for f in TERMS:
        out[f] = normalize(out[f], None if norm_states is None else norm_states[f], update)
    out['total'] = out['recon'] + sum(out[f] * weights[f] for f in TERMS[1:])
    out.update(latents=latents, recon_video=recon_video)
    return out
