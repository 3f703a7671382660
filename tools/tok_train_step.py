"""One training step of the VideoTokenizer mirror on an MI355X: forward + backward time of `VideoTokenizer.forward` at dim 512,
patch 16, 256 x 256 x 3, 8 frames, batch 4 (256 patches + latents per frame: `train_wide_frames=True`), and the pixel-side glue of that step once on
the operators of csrc/tok_train.hip and once composed from torch ops, in the same process.

    timeout -k 10 600 python tools/tok_train_step.py [--out profiles/tok_train_step.txt] [--steps 10] [--warmup 3]

One process, one GPU.  No threshold is asserted: the file is the record."""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dreamer4_amd.tokenizer import VideoTokenizer     # noqa: E402

CFG = dict(dim=512, dim_latent=32, patch_size=16, image_size=256, num_latent_tokens=64, encoder_depth=4, decoder_depth=4, time_block_every=4,
           attn_heads=8, attn_dim_head=64, channels=3, decoder_flow_steps=4, lpips_loss_weight=0., train_wide_frames=True)
B, T = 4, 8


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def glue_hip(tok, video, noise, times, mask, tokens, recon_rows):
    """every pixel-side pass of one step on the new operators, as trunk_ops.tokenizer_losses calls them: both patch embeddings' inputs, both LayerNorms
    with backward, masking with backward, the loss"""
    from dreamer4_amd import trunk_ops as TO
    ps, W = tok.patch_size, dict(tok.named_parameters())
    rows = TO.video_to_patches(video, ps)
    nrows = TO.flow_noised_patches(video, noise, times, ps)
    x = TO.layernorm_nobias(tokens, W['patch_to_tokens.2.weight'], 1e-5)
    x = TO.mask_rows(x, mask, W['mask_token'])
    y = TO.layernorm_nobias(tokens, W['noised_patch_to_tokens.2.weight'], 1e-5)
    loss = TO.recon_loss(recon_rows, video, noise, times, ps, True)
    (loss + (x * y).sum() * 1e-9).backward()
    return rows, nrows


def glue_torch(tok, video, noise, times, mask, tokens, recon_rows):
    """the same passes composed from torch ops (what the reference runs, dreamer4.py:3838-3844, 4344, 4457-4474, 4516)"""
    from torch.nn import functional as F
    ps, W = tok.patch_size, dict(tok.named_parameters())
    b, c, t, H, Wd = video.shape
    nh, nw = H // ps, Wd // ps
    to_rows = lambda v: v.reshape(b, c, t, nh, ps, nw, ps).permute(0, 2, 3, 5, 4, 6, 1).reshape(b, t, nh, nw, ps * ps * c)
    tt = times[:, None, None, None, None]
    noised = noise.lerp(video, tt)
    rows, nrows = to_rows(video).contiguous(), to_rows(noised).contiguous()
    x = F.layer_norm(tokens, tokens.shape[-1:], W['patch_to_tokens.2.weight'], None, 1e-5)
    x = torch.where(mask[..., None], W['mask_token'], x)
    y = F.layer_norm(tokens, tokens.shape[-1:], W['noised_patch_to_tokens.2.weight'], None, 1e-5)
    recon = recon_rows.reshape(b, t, nh, nw, ps, ps, c).permute(0, 6, 1, 2, 4, 3, 5).reshape(b, c, t, H, Wd)
    loss = F.mse_loss((recon - noised) / (1. - tt), video - noise)
    (loss + (x * y).sum() * 1e-9).backward()
    return rows, nrows


def operator_times(tok, video, noise, times, mask, tokens, recon_rows, steps, warmup, reps=20):
    """device time of each operator alone: `reps` back-to-back launches through the C entry points between two events (no Python per launch but ctypes)"""
    import ctypes as C
    from dreamer4_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    W = dict(tok.named_parameters())
    b, c, t, H, Wd = video.shape
    ps = tok.patch_size
    geom = (b, c, t, H // ps, Wd // ps, ps)
    D = tokens.shape[-1]
    rows = tokens.numel() // D
    m8 = mask.to(torch.uint8).contiguous()
    out_v, out_t, dg, loss = torch.empty_like(recon_rows), torch.empty_like(tokens), torch.empty(D, device='cuda'), torch.empty(1, device='cuda')
    nparts = lib.d4_tok_rows_part_floats(rows, D)
    part = torch.empty(max(nparts, 1024), device='cuda')
    g1 = W['patch_to_tokens.2.weight'].detach()
    calls = {
        'video_to_patches (existing kernel)': lambda: lib.d4_video_patches(P(video), P(out_v), *geom, 1, s),
        'flow_noised_patches without noise': lambda: lib.d4_flow_noised_patches(P(video), None, None, P(out_v), *geom, s),
        'flow_noised_patches': lambda: lib.d4_flow_noised_patches(P(video), P(noise), P(times), P(out_v), *geom, s),
        'layernorm_rows (existing kernel)': lambda: lib.d4_layernorm_rows(P(tokens), D, P(g1), None, P(out_t), D, rows, D, 1e-5, 0, s),
        'layernorm_rows_bwd': lambda: lib.d4_layernorm_rows_bwd(P(tokens), D, P(tokens), P(g1), P(out_t), P(dg), P(part), nparts, rows, D, 1e-5, s),
        'mask_rows_fwd': lambda: lib.d4_mask_rows_fwd(P(tokens), P(m8), P(g1), P(out_t), rows, D, s),
        'mask_rows_bwd': lambda: lib.d4_mask_rows_bwd(P(tokens), P(m8), P(out_t), P(dg), P(part), nparts, rows, D, s),
        'recon_loss_fwd_bwd (v-space)': lambda: lib.d4_recon_loss_fwd_bwd(P(recon_rows), P(video), P(noise), P(times), *geom, 1, P(loss), P(out_v), P(part), 1024, s),
    }
    mib = {'video_to_patches (existing kernel)': 2, 'flow_noised_patches without noise': 2, 'flow_noised_patches': 3, 'recon_loss_fwd_bwd (v-space)': 4}
    us = {}
    lines = [f'operators alone, {reps} back-to-back launches each (device time per launch; MiB moved = the minimum the operator must read and write):']
    for name, fn in calls.items():
        def run():
            for _ in range(reps):
                _lib.check(fn())
        med, lo, hi = timed(run, steps, warmup)
        n_mib = (mib[name] * video.numel() if name in mib else (3 if 'bwd' in name else 2) * tokens.numel()) * 4 / 2 ** 20
        us[name] = med / reps * 1e3
        lines.append(f'  {name:36s} {med / reps * 1e3:8.1f} us  ({n_mib:6.1f} MiB -> {n_mib / 1024 / (med / reps * 1e-3):7.1f} GiB/s)')
    # the torch ops each operator stands for, timed the same way (20 back-to-back calls; their kernels are long enough to hide the eager dispatch)
    from torch.nn import functional as F
    nh, nw = H // ps, Wd // ps
    to_rows = lambda v: v.reshape(b, c, t, nh, ps, nw, ps).permute(0, 2, 3, 5, 4, 6, 1).reshape(b, t, nh, nw, ps * ps * c).contiguous()
    tt = times[:, None, None, None, None]
    flat = tokens.reshape(rows, D)
    mean, rstd = flat.mean(-1, keepdim=True), flat.var(-1, unbiased=False, keepdim=True).add(1e-5).rsqrt()
    rr = recon_rows.clone().requires_grad_()

    def loss_chain():
        rr.grad = None
        recon = rr.reshape(b, t, nh, nw, ps, ps, c).permute(0, 6, 1, 2, 4, 3, 5).reshape(b, c, t, H, Wd)
        F.mse_loss((recon - noise.lerp(video, tt)) / (1. - tt), video - noise).backward()

    torch_calls = {
        'rearrange copy (video_to_patches)': lambda: to_rows(video),
        'lerp + rearrange copy (flow_noised_patches)': lambda: to_rows(noise.lerp(video, tt)),
        'F.layer_norm (layernorm_rows)': lambda: F.layer_norm(tokens, (D,), g1, None, 1e-5),
        'native_layer_norm_backward (layernorm_rows_bwd)': lambda: torch.ops.aten.native_layer_norm_backward(flat, flat, [D], mean, rstd, g1, None, [True, True, False]),
        'torch.where (mask_rows_fwd)': lambda: torch.where(mask[..., None], g1, tokens),
        'un-patchify, lerp, mse_loss + autograd (recon_loss_fwd_bwd)': loss_chain,
    }
    lines.append(f'the torch ops they stand for, {reps} back-to-back calls each (time per call):')
    for name, fn in torch_calls.items():
        def run():
            for _ in range(reps):
                fn()
        med, lo, hi = timed(run, steps, warmup)
        us[name] = med / reps * 1e3
        lines.append(f'  {name:60s} {med / reps * 1e3:8.1f} us')
    hip = (us['flow_noised_patches without noise'] + us['flow_noised_patches'] + 2 * us['layernorm_rows (existing kernel)'] + 2 * us['layernorm_rows_bwd']
           + us['mask_rows_fwd'] + us['mask_rows_bwd'] + us['recon_loss_fwd_bwd (v-space)'])
    ref = (us['rearrange copy (video_to_patches)'] + us['lerp + rearrange copy (flow_noised_patches)'] + 2 * us['F.layer_norm (layernorm_rows)']
           + 2 * us['native_layer_norm_backward (layernorm_rows_bwd)'] + 2 * us['torch.where (mask_rows_fwd)']
           + us['un-patchify, lerp, mse_loss + autograd (recon_loss_fwd_bwd)'])
    lines.append(f'one step\'s pixel-side passes added up from the lines above: {hip:.0f} us on the operators, {ref:.0f} us on the torch ops (the mask backward counted as a '
                 'second torch.where).  The glue timed as a whole above is bound by host dispatch in both forms, not by these kernels.')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tok_train_step.txt'))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    torch.manual_seed(0)
    tok = VideoTokenizer(**CFG).cuda().train()
    g = torch.Generator(device='cuda').manual_seed(1)
    video = torch.rand(B, 3, T, 256, 256, device='cuda', generator=g)
    nparam = sum(p.numel() for p in tok.parameters())

    def step():
        tok.zero_grad(set_to_none=True)
        tok(video, generator=g).backward()

    lines = [f'VideoTokenizer training step: {CFG}', f'batch {B}, frames {T}: {video.numel() * 4 / 2 ** 20:.1f} MiB of video, {nparam / 1e6:.1f} M parameters, '
             f'{(256 // 16) ** 2 + CFG["num_latent_tokens"]} tokens per frame, device {torch.cuda.get_device_name(0)}']
    t0 = time.time()
    med, lo, hi = timed(step, a.steps, a.warmup)
    lines.append(f'forward + backward: median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) over {a.steps} steps after {a.warmup} warm-up steps  [{time.time() - t0:.1f} s wall]')
    # the pixel-side glue alone, on leaf inputs of the step's shapes
    noise = torch.randn(video.shape, device='cuda', generator=g)
    times = torch.randint(0, 4, (B,), device='cuda', generator=g).float() / 4
    mask = torch.rand(B, T, 16, 16, device='cuda', generator=g) < 0.45
    tokens = torch.randn(B, T, 16, 16, CFG['dim'], device='cuda', generator=g).requires_grad_()
    recon_rows = torch.randn(B, T, 16, 16, 16 * 16 * 3, device='cuda', generator=g).requires_grad_()

    def glue(fn):
        def run():
            tok.zero_grad(set_to_none=True); tokens.grad = None; recon_rows.grad = None
            fn(tok, video, noise, times, mask, tokens, recon_rows)
        return run

    for name, fn in (('HIP operators (csrc/tok_train.hip)', glue_hip), ('composed from torch ops', glue_torch)):
        med, lo, hi = timed(glue(fn), a.steps, a.warmup)
        lines.append(f'pixel-side glue, {name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})')
    lines += operator_times(tok, video, noise, times, mask, tokens.detach(), recon_rows.detach(), a.steps, a.warmup)
    lines.append('glue = patch rows of the video and of noise.lerp(video, t), both LayerNorms forward + backward on (B T 256) x 512 rows, mask rows forward + backward, '
                 'the v-space reconstruction loss forward + backward; same inputs, same process.  No threshold; no roofline fraction is claimed.')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
