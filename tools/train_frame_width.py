"""Training on wide frames: what the within-frame and cross geometries of the tiled attention core (csrc/attn_tiled.hip) cost.
    python tools/train_frame_width.py            (on an MI355X; the output is profiles/wide_frames_attention.txt)
(a) the space-attention operator alone (forward + backward; dim 512, 8 x 64 heads, 3840 token rows) at 64 tokens per frame on the LDS core
    and, through d4_debug_switch("space_attn_tiled", 1), on the tiled core
(b) the same operator with wide=True at 128 and 256 tokens per frame, the same 3840 rows: time per token row against the tiled 64-token figure
(c) the cross-attention operator (dim and context 512, 8 x 64 heads, 15 groups, wide=True) at nq = 1, nk = 255 and at nq = 32, nk = 256
(d) one flow-only training step of config 2's architecture (bench.py CFG2) with num_spatial_tokens = 64, i.e. 64 + 8 registers + 3 = 75 tokens
    per frame, at 3 x 16 frames (3600 token rows; the bench's step has 3840), next to the bench's own 16 x 16 step at 15 tokens per frame
Timing: 3 warm-up runs, then 7 windows of `reps` runs each between device synchronisations; the figure is the median window.  Every case is
a process of its own under `timeout`; the first failure ends the run."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = 3840


def median_ms(run, reps, windows=7, warm=3):
    import torch
    for _ in range(warm):
        run()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / reps)
    return 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)


def _params(D, Dc, heads, dh, g):
    import torch
    r = lambda *s, k=1.: (torch.randn(*s, generator=g) * k).cuda().requires_grad_()
    hd = heads * dh
    nw = (1. + torch.randn(D, generator=g) * .1).cuda().requires_grad_()
    return r, [nw, r(hd, D, k=3. * D ** -.5), r(hd, Dc, k=Dc ** -.5), r(hd, Dc, k=Dc ** -.5), r(D, hd, k=hd ** -.5), r(heads, D, k=D ** -.5), r(heads, dh, k=.3)]


def space_case(S, tiled):
    import torch
    from dreamer4_amd import _lib, trunk_ops
    F_, D, heads, dh = ROWS // S, 512, 8, 64
    g = torch.Generator().manual_seed(7)
    r, W = _params(D, D, heads, dh, g)
    wm, bm = r(heads, D, k=D ** -.5), r(heads, k=.5)
    x, rv, dy = r(F_, S, D, k=1.5), r(F_, S, heads, dh), r(F_, S, D).detach()
    assert _lib.load().d4_debug_switch(b'space_attn_tiled', int(tiled)) == 0

    def run():
        y = trunk_ops.space_attention(x, *W, residual_values=rv, mix_weight=wm, mix_bias=bm, softclamp_value=50., num_special=1, wide=S > 64)
        y.backward(dy)
    med, lo, hi = median_ms(run, 20)
    core = 'tiled' if (tiled or S > 64) else 'lds'
    return dict(case=f'space attention {F_}x{S} ({core})', S=S, core=core, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                us_per_row=round(1e3 * med / (F_ * S), 4))


def cross_case(nq, nk):
    import torch
    from dreamer4_amd import trunk_ops
    G, D, heads, dh = 15, 512, 8, 64
    g = torch.Generator().manual_seed(13)
    r, W = _params(D, D, heads, dh, g)
    ncw = (1. + torch.randn(D, generator=g) * .1).cuda().requires_grad_()
    q, c, dy = r(G, nq, D, k=1.5), r(G, nk, D, k=1.5), r(G, nq, D).detach()

    def run():
        y = trunk_ops.cross_attention(q, c, W[0], ncw, *W[1:], wide=True)
        y.backward(dy)
    med, lo, hi = median_ms(run, 20)
    return dict(case=f'cross attention {G} x ({nq} over {nk}) (tiled)', nq=nq, nk=nk, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))


def step_case(spatial):
    import torch
    import bench
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    cfg = dict(bench.CFG2, num_spatial_tokens=spatial)
    wide = spatial > 4
    B, T, dev = (3, 16, 'cuda') if wide else (16, 16, 'cuda')
    tokens = 1 + spatial + cfg['num_register_tokens'] + 1 + 1
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**cfg, train_wide_frames=wide)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    lat = torch.randn(B, T, cfg['num_latent_tokens'], cfg['dim_latent'], device=dev, generator=g).clamp(-2, 2)
    acts = torch.randint(0, 4, (B, T, 1), device=dev, generator=g)
    last = []

    def step():
        for p in m.parameters():
            p.grad = None
        total = m(latents=lat, discrete_actions=acts, generator=g, prob_shortcut_train=0.)
        total.backward()
        last[:] = [total]
    med, lo, hi = median_ms(step, 3)
    trunk = [p for k, p in m.named_parameters() if k.startswith('transformer.') and p.grad is not None]
    assert len(trunk) >= 100 and all(torch.isfinite(p.grad).all() for p in trunk) and torch.isfinite(last[0])
    rows = B * T * tokens
    return dict(case=f'flow step {B}x{T}, {tokens} tokens per frame', tokens=tokens, rows=rows, ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2),
                us_per_row=round(1e3 * med / rows, 3), loss=round(last[0].item(), 5))


def child(kind, a, b):
    r = space_case(a, b) if kind == 'space' else cross_case(a, b) if kind == 'cross' else step_case(a)
    print(json.dumps(r), flush=True)


def main():
    cases = [('space', 64, 0), ('space', 64, 1), ('space', 128, 0), ('space', 256, 0), ('cross', 1, 255), ('cross', 32, 256), ('step', 4, 0), ('step', 64, 0)]
    lines, got = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/train_frame_width.py on an MI355X: forward + backward, median of 7 windows after 3 warm-up runs (min .. max of the windows alongside)')
    for kind, a, b in cases:
        p = subprocess.run(['timeout', '-k', '10', '150', sys.executable, os.path.abspath(__file__), kind, str(a), str(b)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} {a} {b}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        say('  '.join(f'{k}={v}' for k, v in r.items()))
    sp = {(r['S'], r['core']): r for r in got if 'core' in r}
    lds, t64 = sp[(64, 'lds')], sp[(64, 'tiled')]
    ratio = t64['ms'] / lds['ms']
    say(f"(a) 64 tokens per frame: tiled {t64['ms']} ms vs LDS core {lds['ms']} ms = {ratio:.3f}x  (expectation: <= 1.10x: {'met' if ratio <= 1.1 else 'NOT met'})")
    for S in (128, 256):
        ratio, bound = sp[(S, 'tiled')]['us_per_row'] / t64['us_per_row'], S / 64.
        say(f"(b) {S} tokens per frame: time per token row {ratio:.3f}x the tiled 64-token figure  (expectation: <= {bound:.0f}x: {'met' if ratio <= bound else 'NOT met'})")
    for r in got:
        if 'nq' in r:
            say(f"(c) cross attention, {r['nq']} queries over {r['nk']} keys, 15 groups: {r['ms']} ms  (no expectation stated{'; one 16-query wave with 15 idle rows per problem' if r['nq'] == 1 else ''})")
    narrow, wide = [r for r in got if 'tokens' in r]
    say(f"(d) flow-only training step, {wide['tokens']} tokens per frame (num_spatial_tokens = 64, train_wide_frames=True): {wide['ms']} ms for {wide['rows']} token rows = "
        f"{wide['us_per_row']} us per row; config 2 itself ({narrow['tokens']} tokens per frame): {narrow['ms']} ms for {narrow['rows']} rows = {narrow['us_per_row']} us per row "
        f"({wide['us_per_row'] / narrow['us_per_row']:.2f}x per row)")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'wide_frames_attention.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
