"""One MuonAdamAtan2 step on an MI355X at the two whole-model sizes the project measures: the dynamics model at config 2's
architecture (dim 512, depth 6; the training step of tools/train_step_time.py, B = T = 16) and the tokenizer of DESIGN.md 20's measurement
(tools/tok_train_step.py).  Per model, in one process, with event windows as tools/tok_train_step.py takes them:

    (i)   MuonAdamAtan2.step() on the kernels of csrc/muon.hip (whole step; Muon group alone; Adam-atan2 group alone), its launch count,
          per-kernel device time of one step (torch profiler), workspace bytes and passes
    (ii)  the same arithmetic composed from torch ops per tensor (torch.matmul per matrix: about 15 launches per Muon matrix)
    (iii) torch.optim.AdamW on the same parameters
    and the training step (forward + backward) the optimiser follows, so the fraction it adds is on record.

    timeout -k 10 900 python tools/muon_step.py [--out profiles/muon_step.txt] [--steps 10] [--warmup 3]

No threshold is asserted: the file is the record."""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dreamer4_amd import DynamicsWorldModel, MuonAdamAtan2, VideoTokenizer, _lib     # noqa: E402
from dreamer4_amd.optim import update_scale                                          # noqa: E402
from dreamer4_amd.synthetic import randomize_weights                                 # noqa: E402

DYN = dict(dim=512, dim_latent=32, num_latent_tokens=32, depth=6, num_discrete_actions=4)
TOK = dict(dim=512, dim_latent=32, patch_size=16, image_size=256, num_latent_tokens=64, encoder_depth=4, decoder_depth=4, time_block_every=4,
           attn_heads=8, attn_dim_head=64, channels=3, decoder_flow_steps=4, lpips_loss_weight=0., train_wide_frames=True)
COEFS = (3.4445, -4.7750, 2.0315)


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


def fmt(t):
    return f'median {t[0]:.3f} ms (min {t[1]:.3f} - max {t[2]:.3f})'


class Naive:
    """the contract of MuonAdamAtan2 from torch ops, tensor by tensor, fp32 on the device"""

    def __init__(self, muon, rest, lr=1e-4, betas=(0.9, 0.99), a=1.27, b=1., beta=0.95):
        self.muon, self.rest, self.lr, self.betas, self.a, self.b, self.beta, self.t = muon, rest, lr, betas, a, b, beta, 0
        self.m = {id(p): torch.zeros_like(p) for p in muon + rest}
        self.v = {id(p): torch.zeros_like(p) for p in rest}

    @torch.no_grad()
    def step_muon(self):
        ca, cb, cc = COEFS
        for p in self.muon:
            m = self.m[id(p)].lerp_(p.grad, 1. - self.beta)
            u = p.grad.lerp(m, self.beta)
            X = u.t() if p.shape[0] > p.shape[1] else u
            X = X / torch.linalg.norm(X).clamp_min(1e-7)
            for _ in range(5):
                A = X @ X.t()
                B = torch.addmm(A, A, A, beta=cb, alpha=cc)
                X = torch.addmm(X, B, X, beta=ca)
            if p.shape[0] > p.shape[1]:
                X = X.t()
            p.add_(X, alpha=-self.lr * update_scale('spectral', *p.shape))

    @torch.no_grad()
    def step_adam(self):
        self.t += 1
        b1, b2 = self.betas
        for p in self.rest:
            m = self.m[id(p)].lerp_(p.grad, 1. - b1)
            v = self.v[id(p)].lerp_(p.grad * p.grad, 1. - b2)
            p.add_(torch.atan2(m / (1. - b1 ** self.t), self.b * (v / (1. - b2 ** self.t)).sqrt()), alpha=-self.lr * self.a)

    def step(self):
        self.step_muon(); self.step_adam()


def kernel_times(fn):
    """device time per kernel name of one call (torch profiler)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, 'device_time_total', None)
        if t is None:
            t = getattr(e, 'cuda_time_total', 0.)
        if t > 0:
            out[e.key] = (t / 1e3, e.count)
    return out


def measure(name, model, train_step, a, lines):
    lib = _lib.load()
    muon = model.muon_parameters()
    ids = {id(p) for p in muon}
    rest = [p for p in model.parameters() if id(p) not in ids and p.numel() > 0]
    g = torch.Generator(device='cuda').manual_seed(7)
    for p in muon + rest:
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-3
    shapes = {}
    for p in muon:
        shapes[tuple(p.shape)] = shapes.get(tuple(p.shape), 0) + 1
    flop = 0
    for p in muon:
        R, C = min(p.shape), max(p.shape)
        flop += 5 * (2 * R * R * C + 2 * R * R * R + 2 * R * R * C)
    lines.append(f'== {name}: {len(muon)} Muon matrices ({sum(p.numel() for p in muon) / 1e6:.1f} M elements; ' +
                 ', '.join(f'{n} x {s[0]}x{s[1]}' for s, n in sorted(shapes.items())) +
                 f'), {len(rest)} Adam-atan2 tensors ({sum(p.numel() for p in rest) / 1e6:.1f} M elements); Newton-Schulz {flop / 1e9:.1f} GFLOP per step '
                 '(full products; the symmetric stages compute the upper tiles only)')
    if train_step is not None:
        keep = {id(p): p.grad for p in muon + rest}
        t_train = timed(train_step, a.steps, a.warmup)
        for p in muon + rest:
            p.grad = keep[id(p)]
        lines.append(f'training step (forward + backward): {fmt(t_train)}')
    opt = MuonAdamAtan2(muon, list(model.parameters()), max_grad_norm=1.)
    t_all = timed(opt.step, a.steps, a.warmup)
    lib.d4_debug_switch(b'launch_count', 0)
    opt.step()
    counted = lib.d4_debug_switch(b'launch_count', 0)
    passes = [lib.d4_muon_plan_passes(plan) for plan, _ in opt._plans.values()]
    lines.append(f'(i)   MuonAdamAtan2.step(), max_grad_norm=1: {fmt(t_all)}; {counted} kernel launches (expected {opt.last_launches}: norm 2, Muon passes x 17, Adam-atan2 1); '
                 f'Muon workspace {opt.muon_workspace_bytes()} bytes ({opt.muon_workspace_bytes() / 2 ** 20:.1f} MiB), passes {passes}')
    if train_step is not None:
        lines.append(f'      = {100 * t_all[0] / t_train[0]:.1f} % on top of the training step')
    kt = kernel_times(opt.step)
    for k, (ms, n) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
        lines.append(f'        {ms:8.3f} ms  x{n:<3d} {k[:110]}')
    if any('muon_gemm' in k for k in kt):
        gemm_ms = sum(ms for k, (ms, n) in kt.items() if 'muon_gemm' in k)
        lines.append(f'        the three product stages together: {gemm_ms:.3f} ms = {flop / gemm_ms / 1e9:.1f} TFLOP/s counting full products')
    opt_m = MuonAdamAtan2(muon, muon)
    opt_a = MuonAdamAtan2([], rest)
    lines.append(f'      Muon group alone:       {fmt(timed(opt_m.step, a.steps, a.warmup))}')
    lines.append(f'      Adam-atan2 group alone: {fmt(timed(opt_a.step, a.steps, a.warmup))}')
    del opt, opt_m, opt_a
    naive = Naive(muon, rest)
    lines.append(f'(ii)  composed from torch ops per tensor: {fmt(timed(naive.step, a.steps, a.warmup))}')
    lines.append(f'      Muon group alone:       {fmt(timed(naive.step_muon, a.steps, a.warmup))}')
    lines.append(f'      Adam-atan2 group alone: {fmt(timed(naive.step_adam, a.steps, a.warmup))}')
    del naive
    adamw = torch.optim.AdamW(muon + rest, lr=1e-4)
    lines.append(f'(iii) torch.optim.AdamW on the same parameters: {fmt(timed(adamw.step, a.steps, a.warmup))}')
    for p in muon + rest:
        assert math.isfinite(float(p.detach().abs().max())), 'a parameter went non-finite'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'muon_step.txt'))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-train', action='store_true', help='skip the training steps (optimiser timings only)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    lines = [f'MuonAdamAtan2 step, device {torch.cuda.get_device_name(0)}; event windows, {a.steps} steps after {a.warmup} warm-up steps, one process']
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**DYN)).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    lat = torch.randn(16, 16, 32, 32, device='cuda', generator=g).clamp(-2, 2)
    acts = torch.randint(0, 4, (16, 16, 1), device='cuda', generator=g)

    def dyn_step():
        m.zero_grad(set_to_none=True)
        m(latents=lat, discrete_actions=acts, generator=g, prob_shortcut_train=0.).backward()

    measure(f'DynamicsWorldModel {DYN}, B = T = 16', m, None if a.no_train else dyn_step, a, lines)
    del m, lat, acts
    torch.cuda.empty_cache()
    tok = VideoTokenizer(**TOK).cuda().train()
    video = torch.rand(4, 3, 8, 256, 256, device='cuda', generator=g)

    def tok_step():
        tok.zero_grad(set_to_none=True)
        tok(video, generator=g).backward()

    measure(f'VideoTokenizer {TOK}, batch 4, 8 frames', tok, None if a.no_train else tok_step, a, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
