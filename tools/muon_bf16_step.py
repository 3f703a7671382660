"""MuonAdamAtan2.step() with muon_products='bf16' against 'fp32' on an MI355X, at the two whole-model sizes of tools/muon_step.py
(DESIGN.md 28): the dynamics model at config 2's architecture and the tokenizer of DESIGN.md 20's measurement.

Per model, in ONE process: one optimiser per mode on the same parameters and gradients, stepped in alternating event windows (fp32, bf16, fp32, ...),
median (min - max) of `--steps` windows after warm-up; then per mode the device time of every Muon kernel of one step (torch profiler), split by stage
(prepare / normalise / gram + poly / apply / finish: the products of an iteration are launched in that order), launches, passes, workspace bytes and
the product throughput counting full products.  The fp32 arm of the same run is the yardstick.

    timeout -k 10 600 python tools/muon_bf16_step.py [--out profiles/muon_bf16.txt] [--steps 10] [--warmup 3]

The file is the record; the one condition asserted is the required one: the 'bf16' step is not slower than the 'fp32' step."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from muon_step import DYN, TOK, fmt                                                  # noqa: E402
from dreamer4_amd import DynamicsWorldModel, MuonAdamAtan2, VideoTokenizer, _lib     # noqa: E402
from dreamer4_amd.synthetic import randomize_weights                                 # noqa: E402

MODES = ('fp32', 'bf16')
STAGES = ('prepare', 'normalise', 'gram + poly', 'apply', 'finish')


def alternating(fns, steps, warmup):
    """{mode: (median, min, max)} of event windows taken in turn: mode 0, mode 1, mode 0, ..."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def stage_times(fn):
    """{stage: ms} of the Muon kernels of one call, and ms of everything else (norm, Adam-atan2), from the device-side events in launch order"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    out, other, nprod = {s: 0. for s in STAGES}, 0., 0
    for e in evs:
        ms = e.time_range.elapsed_us() / 1e3
        if 'muon_prepare' in e.name:
            out['prepare'] += ms
        elif 'normalise' in e.name:
            out['normalise'] += ms
        elif 'muon_finish' in e.name or 'muon_bf16_finish' in e.name:
            out['finish'] += ms
        elif 'muon_gemm' in e.name or 'muon_bf16_gemm' in e.name:
            out['apply' if nprod % 3 == 2 else 'gram + poly'] += ms              # gram, poly, apply per iteration
            nprod += 1
        else:
            other += ms
    return out, other, nprod


def measure(name, model, a, lines):
    lib = _lib.load()
    muon = model.muon_parameters()
    ids = {id(p) for p in muon}
    rest = [p for p in model.parameters() if id(p) not in ids and p.numel() > 0]
    g = torch.Generator(device='cuda').manual_seed(7)
    for p in muon + rest:
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-3
    flop = 0
    for p in muon:
        R, C = min(p.shape), max(p.shape)
        flop += 5 * (2 * R * R * C + 2 * R * R * R + 2 * R * R * C)
    lines.append(f'== {name}: {len(muon)} Muon matrices ({sum(p.numel() for p in muon) / 1e6:.1f} M elements), {len(rest)} Adam-atan2 tensors; '
                 f'Newton-Schulz {flop / 1e9:.1f} GFLOP per step (full products)')
    opts = {mode: MuonAdamAtan2(muon, list(model.parameters()), max_grad_norm=1., muon_products=mode) for mode in MODES}
    t = alternating({mode: opt.step for mode, opt in opts.items()}, a.steps, a.warmup)
    for mode, opt in opts.items():
        lib.d4_debug_switch(b'launch_count', 0)
        opt.step()
        counted = lib.d4_debug_switch(b'launch_count', 0)
        passes = [lib.d4_muon_plan_passes(plan) for plan, _ in opt._plans.values()]
        st, other, nprod = stage_times(opt.step)
        prod = st['gram + poly'] + st['apply']
        lines.append(f"{mode}: step() {fmt(t[mode])}; {counted} kernel launches (expected {opt.last_launches}), passes {passes}, "
                     f"Muon workspace {opt.muon_workspace_bytes()} bytes ({opt.muon_workspace_bytes() / 2 ** 20:.1f} MiB)")
        lines.append('      device time of one step: ' + ', '.join(f'{s} {st[s]:.3f} ms' for s in STAGES) + f'; norm + Adam-atan2 {other:.3f} ms')
        lines.append(f'      the {nprod} product launches together: {prod:.3f} ms = {flop / max(prod, 1e-9) / 1e9:.1f} TFLOP/s counting full products')
    lines.append(f"bf16 / fp32 step: {t['bf16'][0] / t['fp32'][0]:.3f}")
    for p in muon + rest:
        assert torch.isfinite(p.detach()).all(), 'a parameter went non-finite'
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'muon_bf16.txt'))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    lines = [f'MuonAdamAtan2 step, muon_products fp32 | bf16, device {torch.cuda.get_device_name(0)}; alternating event windows, {a.steps} steps per mode '
             f'after {a.warmup} warm-up steps, one process']
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**DYN)).cuda()
    got = {'dynamics': measure(f'DynamicsWorldModel {DYN}', m, a, lines)}
    del m
    torch.cuda.empty_cache()
    tok = VideoTokenizer(**TOK).cuda().train()
    got['tokenizer'] = measure(f'VideoTokenizer {TOK}', tok, a, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    for k, t in got.items():
        assert t['bf16'][0] <= t['fp32'][0], f"{k}: the bf16 step ({t['bf16'][0]:.3f} ms) is slower than the fp32 step ({t['fp32'][0]:.3f} ms)"


if __name__ == '__main__':
    main()
