"""The latent regularisers of the VideoTokenizer training forward on an MI355X, at the tokenizer architecture of DESIGN.md 20
(dim 512, 64 latents x 32, patch 16, 256 x 256 x 3):

  * the SIGReg operator (d4_sigreg_fwd_bwd: loss and gradient in one call) against the reference's formulation composed from torch ops (a complex
    tensor of batch x (frames . latents) x slices x knots, forward + autograd backward), 256 slices, 17 knots, 16 frames per clip, at the largest
    batch of --batches at which the composed form runs; time and peak memory of both, and the difference of their results;
  * the orthogonality operator against the composed torch form, the same way;
  * one training step (forward + backward, batch 4 x 8 frames) with each term on and with all three, against the same step with all weights 0.

    timeout -k 10 900 python tools/tok_reg_step.py [--out profiles/tok_regularisers.txt] [--steps 10] [--warmup 3]

One process, one GPU.  No threshold is asserted: the file is the record."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from dreamer4_amd import trunk_ops                     # noqa: E402
from dreamer4_amd.tokenizer import VideoTokenizer     # noqa: E402
from tok_train_step import CFG, B, T, timed            # noqa: E402

SLICES, KNOTS, DOMAIN, FRAMES = 256, 17, (-5., 5.), 16


def complex_sigreg(x, projs):
    """sigreg as the reference evaluates it (dreamer4.py:728-767), composed from torch ops"""
    u = torch.nn.functional.normalize(projs, dim=-1)
    t = torch.linspace(*DOMAIN, KNOTS, device=x.device)
    phi = (-0.5 * t.square()).exp()
    x_t = torch.einsum('knd,md->knm', x.reshape(x.shape[0], -1, x.shape[-1]), u)[..., None] * t
    ecf = (1j * x_t).exp().mean(dim=1)
    return torch.trapz((ecf - phi).abs().square() * phi, t, dim=-1).mean()


def torch_ortho(x):
    """orthogonal_loss as the reference evaluates it (dreamer4.py:389-402)"""
    n = x.shape[-2]
    y = torch.nn.functional.normalize(x - x.mean(dim=-2, keepdim=True), dim=-1)
    sim = (y @ y.transpose(-1, -2)).masked_fill(torch.eye(n, device=x.device, dtype=torch.bool), 0.)
    return sim.square().sum(dim=(-1, -2)).mean()


def fwd_bwd(loss_fn, x):
    def run():
        x.grad = None
        loss_fn(x).backward()
    return run


def measure(name, loss_fn, x, steps, warmup):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    med, lo, hi = timed(fwd_bwd(loss_fn, x), steps, warmup)
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    x.grad = None
    loss = loss_fn(x)
    loss.backward()
    return f'  {name:46s} median {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   peak memory above the inputs {peak:10.1f} MiB', loss.detach(), x.grad.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tok_regularisers.txt'))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 16, 8, 4, 2, 1])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    g = torch.Generator(device='cuda').manual_seed(1)
    n_lat, d_lat = CFG['num_latent_tokens'], CFG['dim_latent']
    lines = [f'latent regularisers of the VideoTokenizer training forward, device {torch.cuda.get_device_name(0)}',
             f'command: python tools/tok_reg_step.py --steps {a.steps} --warmup {a.warmup} --batches {" ".join(map(str, a.batches))}',
             f'SIGReg: {FRAMES} frames x {n_lat} latents x {d_lat} per clip, {SLICES} slices, {KNOTS} knots on {DOMAIN}; forward + backward, time per call by device events']
    projs = torch.randn(SLICES, d_lat, device='cuda', generator=g)
    for batch in a.batches:
        x = (torch.randn(batch, FRAMES, n_lat, d_lat, device='cuda', generator=g) * 1.5).requires_grad_()
        elems = batch * FRAMES * n_lat * SLICES * KNOTS
        try:
            ref_line, ref_loss, ref_dx = measure('composed from torch ops (complex64)', lambda v: complex_sigreg(v, projs), x, a.steps, a.warmup)
        except torch.cuda.OutOfMemoryError:
            lines.append(f'batch {batch}: the composed form does not fit ({elems:.2e} complex64 elements per intermediate)')
            torch.cuda.empty_cache()
            continue
        op_line, loss, dx = measure('d4_sigreg_fwd_bwd (csrc/tok_reg.hip)', lambda v: trunk_ops.sigreg(v, projs, DOMAIN, KNOTS), x, a.steps, a.warmup)
        lines += [f'batch {batch} ({elems:.2e} complex64 elements = {elems * 8 / 2 ** 30:.2f} GiB per intermediate of the composed form):', ref_line, op_line,
                  f'  results: loss {loss.item():.6e} against {ref_loss.item():.6e}; gradient max |difference| {(dx - ref_dx).abs().max().item():.3e} at max |gradient| '
                  f'{ref_dx.abs().max().item():.3e}']
        break
    x = torch.randn(B * 8 * FRAMES, n_lat, d_lat, device='cuda', generator=g).tanh().requires_grad_()
    lines.append(f'orthogonality: {x.shape[0]} frames x {n_lat} latents x {d_lat}; forward + backward')
    ref_line, ref_loss, ref_dx = measure('composed from torch ops', torch_ortho, x, a.steps, a.warmup)
    op_line, loss, dx = measure('d4_latent_ortho_fwd_bwd (csrc/tok_reg.hip)', trunk_ops.latent_ortho, x, a.steps, a.warmup)
    lines += [ref_line, op_line, f'  results: loss {loss.item():.6e} against {ref_loss.item():.6e}; gradient max |difference| {(dx - ref_dx).abs().max().item():.3e} at max '
              f'|gradient| {ref_dx.abs().max().item():.3e}']

    video = torch.rand(B, 3, T, 256, 256, device='cuda', generator=g)
    lines.append(f'training step, forward + backward, batch {B} x {T} frames, {CFG}; each tokenizer from the same seed, in this process, in this order:')
    terms = dict(latent_sigreg_loss_weight=0.1, latent_ortho_loss_weight=0.1, latent_consistency_loss_weight=0.1)
    base = None
    for name, extra in [('all weights 0', {}), *[(k + ' = 0.1', {k: v}) for k, v in terms.items()], ('all three = 0.1', terms), ('all weights 0 again', {})]:
        torch.manual_seed(0)
        tok = VideoTokenizer(**CFG, **extra).cuda().train()

        def step():
            tok.zero_grad(set_to_none=True)
            tok(video, generator=g).backward()

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        med, lo, hi = timed(step, a.steps, a.warmup)
        base = med if base is None else base
        lines.append(f'  {name:38s} median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f})  {med / base:5.2f} x the first line   peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:6.2f} GiB')
        del tok
    lines.append('The consistency term is a second encoder pass (forward and backward) on the decoder output.  No threshold; no roofline fraction is claimed.')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
