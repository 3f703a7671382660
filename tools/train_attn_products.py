"""Training attention on the bf16 matrix pipe: what the bf16-product form of the tiled core (csrc/attn_tiled_bf16.hip) buys.
    python tools/train_attn_products.py            (on an MI355X; the output is profiles/train_attn_bf16.txt)
(a) the core alone through the operator entries (d4_train_attn_core with core 1, which this option leaves untouched and so stands for the fp32
    products, against d4_train_attn_core_bf16), forward only and forward + backward, 8 x 64 heads, clamp 50, value residual and belief on,
    about 3840 rows: the time geometry at 256, 512 and 1024 frames, the within-frame geometry at 256 and 1024 tokens; at 256 items also head
    dims 32 and 16 (recorded only)
(b) the time-attention operator (config 2's geometry: 15 tokens, dim 512, 8 x 64 heads), forward + backward, at 2 x 192 and 1 x 1024 frames
(c) a flow-only training step of config 2's architecture at 2 x 192 frames, train_attn_products 'fp32' against 'bf16'
(d) the same with num_spatial_tokens=256 and train_wide_frames=True, in both train_matmul_dtype modes, at 1 x 192 frames (51k token rows): at
    2 x 192 the saved forward workspaces of a step exceed the 288 GB of the device (HIP out of memory, tried once)
Timing: both arms of a comparison in one process, their windows alternating; warm-up runs, then 7 windows of `reps` runs each between device
synchronisations; the figure is the median window.  Every case is a process of its own under `timeout`; the first failure ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from infer_frame_width import ROWS, median_ms  # noqa: E402


def core_case(geo, items, dh):
    import torch
    from dreamer4_amd import _lib
    lib = _lib.load()
    H, groups = 8, max(1, ROWS // items)
    hd, hp4, rows = H * dh, 8, groups * items
    ldp = 3 * hd + hp4 + H
    g = torch.Generator().manual_seed(7)
    r = lambda *s, k=1.: (torch.randn(*s, generator=g) * k).cuda()
    proj, rv, gamma, d_o3 = r(rows, ldp), r(rows, hd), r(hd, k=.3), r(rows, hd)
    proj[:, :hd] *= 3
    time = geo == 'time'
    inv_freq = (1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))).cuda() if time else None
    geom = (groups, items * groups, groups) if time else (1, items, 1)              # g_inner, g_outer_stride, item_stride
    pf = [lib.d4_train_attn_core_plane_floats(rows, H, dh), lib.d4_train_attn_core_bf16_plane_floats(groups, items, H, dh)]
    planes = [torch.empty(n, device='cuda') for n in pf]
    outs = [dict(o3=torch.empty(rows, hd, device='cuda'), dproj=torch.zeros(rows, ldp, device='cuda'), d_rv=torch.empty(rows, hd, device='cuda'),
                 dgamma=torch.empty(groups, hd, device='cuda')) for _ in range(2)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _lib.ptr
    fns = [lib.d4_train_attn_core, lib.d4_train_attn_core_bf16]

    def arm(a, backward):
        o = outs[a]

        def run():
            _lib.check(fns[a](P(proj), ldp, P(rv), P(gamma), P(d_o3) if backward else None, P(o['o3']), P(o['dproj']), P(o['d_rv']), P(o['dgamma']),
                              groups, items, H, dh, 50., 0 if time else 1, 1, *geom, int(time), P(inv_freq) if time else None, 1, P(planes[a]), pf[a], stream))
        return run
    fwd, reps_f = median_ms([arm(0, False), arm(1, False)])
    both, reps_b = median_ms([arm(0, True), arm(1, True)])
    rel = lambda n: (outs[0][n] - outs[1][n]).abs().max().item() / outs[0][n].abs().max().item()
    diff = {n: rel(n) for n in ('o3', 'dproj', 'd_rv', 'dgamma')}
    assert all(0. < d < 0.1 for d in diff.values()), diff
    rd = lambda x: round(x, 4)
    return dict(case=f'{geo} core {groups}x{items}, 8 x {dh} heads', geo=geo, items=items, dh=dh, rows=rows, reps=(reps_f, reps_b),
                fp32_form=lib.d4_debug_last_form(b'train_attn').decode(), bf16_form=lib.d4_debug_last_form(b'train_attn_bf16').decode(),
                fp32_fwd_ms=rd(fwd[0][0]), bf16_fwd_ms=rd(fwd[1][0]), fp32_ms=rd(both[0][0]), fp32_ms_min=rd(both[0][1]), fp32_ms_max=rd(both[0][2]),
                bf16_ms=rd(both[1][0]), bf16_ms_min=rd(both[1][1]), bf16_ms_max=rd(both[1][2]), rel_diff_o3=float(f"{diff['o3']:.2e}"),
                rel_diff_dproj=float(f"{diff['dproj']:.2e}"))


def op_case(B, T):
    import torch
    from dreamer4_amd import trunk_ops
    S, D, heads, dh = 15, 512, 8, 64
    g = torch.Generator().manual_seed(9)
    r = lambda *s, k=1.: (torch.randn(*s, generator=g) * k).cuda().requires_grad_()
    hd = heads * dh
    W = [1. + r(D, k=.1).detach(), r(hd, D, k=3. * D ** -.5), r(hd, D, k=D ** -.5), r(hd, D, k=D ** -.5), r(D, hd, k=hd ** -.5), r(heads, D, k=D ** -.5), r(heads, dh, k=.3)]
    W[0].requires_grad_()
    wm, bm = r(heads, D, k=D ** -.5), r(heads, k=.5)
    x, rv, dy = r(B, T, S, D, k=1.5), r(B, T, S, heads, dh), r(B, T, S, D).detach()
    inv_freq = (1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))).cuda()

    def arm(prod):
        def run():
            y = trunk_ops.time_attention(x, *W, inv_freq, residual_values=rv, mix_weight=wm, mix_bias=bm, softclamp_value=50., attn_products=prod)
            y.backward(dy)
        return run
    res, reps = median_ms([arm('fp32'), arm('bf16')])
    rd = lambda v: round(v, 3)
    return dict(case=f'time attention operator {B}x{T} frames, 15 tokens, dim 512, 8 x 64 heads, forward + backward', op=f'{B}x{T}', reps=reps,
                fp32_ms=rd(res[0][0]), fp32_ms_min=rd(res[0][1]), fp32_ms_max=rd(res[0][2]), bf16_ms=rd(res[1][0]), bf16_ms_min=rd(res[1][1]), bf16_ms_max=rd(res[1][2]))


def step_case(wide, arith):
    import torch
    import bench
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    B, T = (1, 192) if wide else (2, 192)
    extra = dict(num_spatial_tokens=256, train_wide_frames=True) if wide else {}
    cfg = dict(bench.CFG2, train_matmul_dtype=('fp32', 'bf16')[arith], **extra)
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**cfg)).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    lat = torch.randn(B, T, cfg['num_latent_tokens'], cfg['dim_latent'], device='cuda', generator=g).clamp(-2, 2)
    acts = torch.randint(0, 4, (B, T, 1), device='cuda', generator=g)
    last = {}

    def arm(prod):
        def run():
            m.train_attn_products = prod
            for p in m.parameters():
                p.grad = None
            total = m(latents=lat, discrete_actions=acts, generator=g, prob_shortcut_train=0.)
            total.backward()
            last[prod] = total
        return run
    res, reps = median_ms([arm('fp32'), arm('bf16')], windows=7, warm=2, window_s=0.3)
    assert all(torch.isfinite(v) for v in last.values())
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
    rd = lambda v: round(v, 2)
    what = f"num_spatial_tokens=256, train_wide_frames=True, train_matmul_dtype={cfg['train_matmul_dtype']}" if wide else "config 2's architecture"
    return dict(case=f'flow-only training step {B}x{T} frames, {what}', step='d' if wide else 'c', arith=cfg['train_matmul_dtype'], reps=reps,
                fp32_ms=rd(res[0][0]), fp32_ms_min=rd(res[0][1]), fp32_ms_max=rd(res[0][2]), bf16_ms=rd(res[1][0]), bf16_ms_min=rd(res[1][1]), bf16_ms_max=rd(res[1][2]),
                loss_fp32=round(last['fp32'].item(), 5), loss_bf16=round(last['bf16'].item(), 5))


def child(kind, a, b):
    r = core_case('time' if kind == 'time' else 'frame', a, b) if kind in ('time', 'frame') else op_case(a, b) if kind == 'op' else step_case(a, b)
    print(json.dumps(r), flush=True)


def main():
    cases = [('time', 256, 64), ('time', 512, 64), ('time', 1024, 64), ('frame', 256, 64), ('frame', 1024, 64), ('time', 256, 32), ('time', 256, 16),
             ('frame', 256, 32), ('frame', 256, 16), ('op', 2, 192), ('op', 1, 1024), ('step', 0, 0), ('step', 1, 0), ('step', 1, 1)]
    lines, got = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/train_attn_products.py on an MI355X: median of 7 windows after warm-up (min .. max of the windows alongside); fp32 = d4_train_attn_core / '
        "attn_products='fp32' (code this option does not touch), bf16 = d4_train_attn_core_bf16 / attn_products='bf16'")
    for kind, a, b in cases:
        p = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), kind, str(a), str(b)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} {a} {b}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        say('  '.join(f'{k}={v}' for k, v in r.items()))
    for r in got:
        if 'geo' in r:
            fb, fw = r['bf16_ms'] / r['fp32_ms'], r['bf16_fwd_ms'] / r['fp32_fwd_ms']
            if r['dh'] == 64:
                note = f"required: not slower: {'met' if fb <= 1. and fw <= 1. else 'NOT met'}"
                if r['items'] == 1024:
                    note += f"; expected: forward + backward <= 0.6x: {'met' if fb <= .6 else 'NOT met'}"
            else:
                note = 'recorded only'
            say(f"(a) {r['geo']} geometry, {r['items']} items, head dim {r['dh']}: forward {r['bf16_fwd_ms']} vs {r['fp32_fwd_ms']} ms = {fw:.3f}x; forward + backward "
                f"{r['bf16_ms']} vs {r['fp32_ms']} ms = {fb:.3f}x  ({note})")
    for r in got:
        if 'op' in r:
            say(f"(b) {r['case']}: attn_products='bf16' {r['bf16_ms']} ms vs 'fp32' {r['fp32_ms']} ms = {r['bf16_ms'] / r['fp32_ms']:.3f}x")
        if 'step' in r:
            say(f"({r['step']}) {r['case']}: train_attn_products='bf16' {r['bf16_ms']} ms vs 'fp32' {r['fp32_ms']} ms = {r['bf16_ms'] / r['fp32_ms']:.3f}x")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'train_attn_bf16.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
