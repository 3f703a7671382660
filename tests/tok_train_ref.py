"""Plain-torch references of the tokenizer's training forward: the four pixel-side operators of csrc/tok_train.hip written out, and the whole
forward (dreamer4.py:4239-4603, the supported subset) composed from the blocks of oracle/restate.py under autograd.

Every operator reference takes `dtype`: float64 is the yardstick; float32 is the same formula in the kernels' number format with every column sum
and the loss sum added strictly one term after the other (tests/tok_train_cases.py derives the tolerance from the two)."""
import numpy as np
import torch

from oracle import restate


def seq_sum0(x, dtype):
    """sum over dim 0; in float32 the terms are added in order"""
    if dtype == torch.float64:
        return x.sum(dim=0)
    return torch.from_numpy(np.asarray(np.cumsum(x.numpy().astype(np.float32), axis=0, dtype=np.float32)[-1]).copy())


def patch_rows(video, ps):
    """'b c t (h p1) (w p2) -> b t h w (p1 p2 c)'  (dreamer4.py:3838-3844, 3896)"""
    b, c, t, H, W = video.shape
    nh, nw = H // ps, W // ps
    return video.reshape(b, c, t, nh, ps, nw, ps).permute(0, 2, 3, 5, 4, 6, 1).reshape(b, t, nh, nw, ps * ps * c)


def rows_to_video(rows, c, ps):
    """'b t h w (p1 p2 c) -> b c t (h p1) (w p2)'  (dreamer4.py:3556)"""
    b, t, nh, nw, _ = rows.shape
    return rows.reshape(b, t, nh, nw, ps, ps, c).permute(0, 6, 1, 2, 4, 3, 5).reshape(b, c, t, nh * ps, nw * ps)


def _tt(times, ndim, dtype):
    return times.to(dtype).reshape(-1, *([1] * (ndim - 1)))


def flow_noised_patches_ref(video, noise, times, ps, *, dtype=torch.float64):
    """patch rows of noise.lerp(video, t[b])  (dreamer4.py:4457)"""
    v, n = video.to(dtype), noise.to(dtype)
    return patch_rows(torch.lerp(n, v, _tt(times, 5, dtype)), ps)


def layernorm_rows_bwd_ref(x, dy, g, eps, *, dtype=torch.float64):
    """y = xhat g, xhat = (x - mean) rstd (biased variance) -> (dx, dg)"""
    x, dy, g = x.to(dtype), dy.to(dtype), g.to(dtype)
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    rstd = torch.rsqrt(xc.pow(2).mean(dim=-1, keepdim=True) + eps)
    xhat = xc * rstd
    gd = g * dy
    dx = rstd * (gd - gd.mean(dim=-1, keepdim=True) - xhat * (gd * xhat).mean(dim=-1, keepdim=True))
    return dx, seq_sum0(dy * xhat, dtype)


def mask_rows_fwd_ref(x, mask, token):
    return torch.where(mask[..., None], token, x)


def mask_rows_bwd_ref(dy, mask, *, dtype=torch.float64):
    dy = dy.to(dtype)
    m = mask[..., None]
    return torch.where(m, torch.zeros_like(dy), dy), seq_sum0(torch.where(m, dy, torch.zeros_like(dy)).reshape(-1, dy.shape[-1]), dtype)


def recon_loss_ref(recon_rows, video, noise, times, ps, v_space, *, dtype=torch.float64):
    """(mean squared error, d loss / d recon_rows); v-space: pred = (recon - noised) / (1 - t), target = video - noise  (dreamer4.py:4469-4474, 4516)"""
    r, v = recon_rows.to(dtype), patch_rows(video.to(dtype), ps)
    n_el = r.numel()
    if v_space:
        n = patch_rows(noise.to(dtype), ps)
        tt = _tt(times, 5, dtype)
        diff = (r - torch.lerp(n, v, tt)) / (1. - tt) - (v - n)
        scale = 1. / (1. - tt)
    else:
        diff, scale = r - v, 1.
    loss = seq_sum0((diff * diff).reshape(-1), dtype) / n_el
    return loss, (2. / n_el) * diff * scale


# ----------------------------------------------------------------------------- the whole training forward
def encoder_latents(tc, W, video, patch_mask=None):
    """dreamer4.py:4309-4425 with MAE masking: video (b, c, t, H, W) -> latents (b, t, n, dim_latent)"""
    b, c, t = video.shape[:3]
    x = patch_rows(video, tc.patch_size)
    x = x @ W['patch_to_tokens.1.weight'].t() + W['patch_to_tokens.1.bias']
    x = restate.layernorm(x, W['patch_to_tokens.2.weight'], 0.)
    if patch_mask is not None:
        x = torch.where(patch_mask[..., None], W['mask_token'], x)                                           # dreamer4.py:4344
    x = x.reshape(b, t, -1, tc.dim)
    tokens = torch.cat((x, W['latent_tokens'].expand(b, t, -1, -1)), dim=2)
    tokens, _ = restate.transformer(tc.encoder_trunk(), W, tokens, None, pre='encoder_transformer.', num_special=tc.num_latent_tokens)
    return (tokens[:, :, x.shape[2]:] @ W['encoded_to_latents.weight'].t()).tanh()


def decoder_rows(tc, W, latents, noised_video, time_indices):
    """decode_step (dreamer4.py:4137-4184, 3599-3682) with one time index per clip -> patch rows (b, t, nh, nw, p1 p2 c)"""
    b, t = latents.shape[:2]
    p = tc.patch_size
    nh, nw = tc.image_height // p, tc.image_width // p
    lat = latents @ W['latents_to_decoder.weight'].t() + W['time_embed.weight'][time_indices][:, None, None]
    x = patch_rows(noised_video, p)
    x = x @ W['noised_patch_to_tokens.1.weight'].t() + W['noised_patch_to_tokens.1.bias']
    x = restate.layernorm(x, W['noised_patch_to_tokens.2.weight'], 0.)
    gy, gx = torch.meshgrid(torch.linspace(-1., 1., nh), torch.linspace(-1., 1., nw), indexing='ij')
    grid = torch.stack((gy, gx), dim=-1).to(x.dtype)
    pos = restate.mlp(W, 'decoder.to_decoder_pos_emb.', grid, restate.mlp_num_layers(tc.decoder_pos_mlp_depth), tc.head_mlp_recipe)
    tokens = torch.cat(((pos + x).reshape(b, t, nh * nw, tc.dim), lat), dim=2)
    tokens, _ = restate.transformer(tc.trunk(), W, tokens, None, pre='decoder.transformer.')
    rows = tokens[:, :, :nh * nw] @ W['decoder.tokens_to_patch.0.weight'].t() + W['decoder.tokens_to_patch.0.bias']
    return rows.reshape(b, t, nh, nw, -1)


def training_forward(tc, W, video, draws, *, v_space=True, norm_state=None, update=True):
    """VideoTokenizer.forward (dreamer4.py:4239-4603) for the supported subset, in the dtype of `video` and W.  draws: patch_mask (b, t, nh, nw) bool
    or None, time_indices (b,), noise.  norm_state: None (no loss normalisation) or the running mean square (1,), updated in place when `update`.
    -> dict(recon, total, latents, recon_video)"""
    latents = encoder_latents(tc, W, video, draws.get('patch_mask'))
    ti, noise = draws['time_indices'], draws['noise'].to(video.dtype)
    times = ti.to(video.dtype) / tc.decoder_flow_steps
    tt = times[:, None, None, None, None]
    noised = torch.lerp(noise, video, tt)
    recon_video = rows_to_video(decoder_rows(tc, W, latents, noised, ti), tc.channels, tc.patch_size)
    if v_space:
        pred, target = (recon_video - noised) / (1. - tt), video - noise
    else:
        pred, target = recon_video, video
    recon = (pred - target).pow(2).mean()
    if norm_state is not None:                                                                                # LossNormalizer, dreamer4.py:645-669
        rms = norm_state.sqrt()
        if update:
            norm_state.lerp_(recon.detach().reshape(1).square().to(norm_state.dtype), 1. - 0.95)
        recon = recon / rms.clamp(min=1e-6).reshape(())
    return dict(recon=recon, total=recon, latents=latents, recon_video=recon_video)


def tokenizer_config(kw):
    return restate.TokenizerConfig(**kw)


def double_weights(W):
    """float64 leaves with gradient for every floating-point parameter (the rotary frequencies are a buffer)"""
    return {k: (v.double().requires_grad_() if v.is_floating_point() and 'inv_freq' not in k else v.double()) for k, v in W.items()}
