"""Training on long clips: what the tiled time-attention core (csrc/attn_tiled.hip) costs, at a constant 384 frames per step.
    python tools/train_clip_length.py
(a) the config-2 training step (bench.py train_flow_step's model, flow only) at B x T = 24x16, 6x64, 3x128, 2x192; at T = 192 every trunk
    gradient is checked to be there and finite
(b) the time-attention operator alone (forward + backward, config 2's geometry: 15 tokens, dim 512, 8 x 64 heads) at T = 64 on the LDS core
    and, through d4_debug_switch("time_attn_tiled", 1), on the tiled core
(c) the same operator at T = 128 and T = 192: per-frame time against the tiled T = 64 figure and the causal work ratio (T + 1) / 65
Every timed case is a process of its own under `timeout`; the first failure ends the run."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = 384


def step_case(T):
    import torch
    import bench
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    B, dev = FRAMES // T, 'cuda'
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**bench.CFG2)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    lat = torch.randn(B, T, bench.CFG2['num_latent_tokens'], bench.CFG2['dim_latent'], device=dev, generator=g).clamp(-2, 2)
    acts = torch.randint(0, 4, (B, T, 1), device=dev, generator=g)

    def step(lat=lat, acts=acts):
        for p in m.parameters():
            p.grad = None
        total = m(latents=lat, discrete_actions=acts, generator=g, prob_shortcut_train=0.)
        total.backward()
        return total
    # the trunk parameters on the path (a cross attention's value-residual mix, for one, is constructed and never used): those a 4-frame step reaches
    step(lat[:1, :4].contiguous(), acts[:1, :4].contiguous())
    on_path = [k for k, p in m.named_parameters() if k.startswith('transformer.') and p.grad is not None]
    for _ in range(2):
        total = step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    reps = 4
    for _ in range(reps):
        step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / reps
    own = dict(m.named_parameters())
    trunk = {k: own[k] for k in on_path}
    missing = [k for k, p in trunk.items() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert len(trunk) >= 100 and not missing and torch.isfinite(total), (len(trunk), missing)
    return dict(case=f'step {B}x{T}', ms=round(1e3 * dt, 2), frames_per_sec=round(FRAMES / dt, 1), loss=round(total.item(), 5), trunk_grads=len(trunk))


def op_case(T, tiled):
    import torch
    from dreamer4_amd import _lib, trunk_ops
    B, S, D, heads, dh = FRAMES // T, 15, 512, 8, 64
    g = torch.Generator().manual_seed(9)
    r = lambda *s, k=1.: (torch.randn(*s, generator=g) * k).cuda().requires_grad_()
    hd = heads * dh
    W = [1. + r(D, k=.1).detach(), r(hd, D, k=3. * D ** -.5), r(hd, D, k=D ** -.5), r(hd, D, k=D ** -.5), r(D, hd, k=hd ** -.5), r(heads, D, k=D ** -.5), r(heads, dh, k=.3)]
    W[0].requires_grad_()
    wm, bm = r(heads, D, k=D ** -.5), r(heads, k=.5)
    x, rv, dy = r(B, T, S, D, k=1.5), r(B, T, S, heads, dh), r(B, T, S, D).detach()
    inv_freq = (1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))).cuda()
    lib = _lib.load()
    assert lib.d4_debug_switch(b'time_attn_tiled', int(tiled)) == 0

    def run():
        y = trunk_ops.time_attention(x, *W, inv_freq, residual_values=rv, mix_weight=wm, mix_bias=bm, softclamp_value=50.)
        y.backward(dy)
    for _ in range(3):
        run()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        run()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / reps
    core = 'tiled' if (tiled or T > 64) else 'lds'
    return dict(case=f'time attention {B}x{T} ({core})', T=T, core=core, ms=round(1e3 * dt, 3), us_per_frame=round(1e6 * dt / FRAMES, 3))


def child(kind, T, tiled):
    print(json.dumps(step_case(T) if kind == 'step' else op_case(T, tiled)), flush=True)


def main():
    cases = [('step', 16, 0), ('step', 64, 0), ('step', 128, 0), ('step', 192, 0), ('op', 64, 0), ('op', 64, 1), ('op', 128, 0), ('op', 192, 0)]
    got = []
    for kind, T, tiled in cases:
        p = subprocess.run(['timeout', '-k', '10', '150', sys.executable, os.path.abspath(__file__), kind, str(T), str(tiled)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} T={T} tiled={tiled}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        print('  '.join(f'{k}={v}' for k, v in r.items()), flush=True)
    ops = {(r['T'], r['core']): r for r in got if 'core' in r}
    lds, t64 = ops[(64, 'lds')], ops[(64, 'tiled')]
    print(f"(b) T=64: tiled {t64['ms']} ms vs LDS core {lds['ms']} ms = {t64['ms'] / lds['ms']:.3f}x  (expectation: <= 1.10x)")
    for T in (128, 192):
        ratio, bound = ops[(T, 'tiled')]['us_per_frame'] / t64['us_per_frame'], (T + 1) / 65.
        print(f"(c) T={T}: per-frame time {ratio:.3f}x the tiled T=64 figure  (expectation: <= {bound:.3f}x, the causal work ratio)")
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
