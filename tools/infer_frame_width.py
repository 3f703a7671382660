"""Wide frames in inference: what the tiled matrix-pipe attention core (csrc/attn_wide_mfma.hip) costs.
    python tools/infer_frame_width.py            (on an MI355X; the output is profiles/wide_frames_inference.txt)
(a) self attention with belief projection and value residual (8 x 64 heads, 3840 token rows in all) at 128 and 160 tokens per frame:
    attn_wide_kernel through d4_small_attn (the yardstick) against wide_attn_kernel<64> through d4_small_attn_wide
(b) the same operator at 64 tokens per frame, head dims 64 and 16: the form the launcher picks today against the new core forced by
    d4_debug_switch("small_attn_wide", 1)
(c) the new core at 256, 512 and 1024 tokens per frame: time per token row against the forced 64-token figure of (b) (bound: S / 64 x)
(d) generate() with config 2's architecture (bench.py CFG2) at num_spatial_tokens 64 and 256 with wide_frames=True, the batch chosen so that
    the token rows per step match config 2's 256 x 15, next to config 2's own step in the same run
Timing: both arms of a comparison in one process, their windows alternating; 3 warm-up runs, then 7 windows of `reps` runs each between
device synchronisations (reps calibrated to ~0.1 s per window); the figure is the median window.  Every case is a process of its own under
`timeout`; the first failure ends the run."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = 3840


def median_ms(runs, windows=7, warm=3, window_s=0.1):
    """runs: the arms of one comparison -> (median, min, max) ms per arm; the arms' windows alternate"""
    import torch
    for run in runs:
        for _ in range(warm):
            run()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10):
        runs[0]()
    torch.cuda.synchronize()
    reps = max(3, int(window_s / max((time.perf_counter() - t0) / 10, 1e-6)))
    ts = [[] for _ in runs]
    for _ in range(windows):
        for a, run in enumerate(runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                run()
            torch.cuda.synchronize(); ts[a].append((time.perf_counter() - t0) / reps)
    return [(1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)) for t in ts], reps


def attn_case(S, dh, forced):
    """self attention, belief + value residual, 8 heads: today's form (d4_small_attn) against the wide core (d4_small_attn_wide)"""
    import torch
    from dreamer4_amd import _lib
    lib = _lib.load()
    G, H = max(1, ROWS // S), 8
    hd = H * dh
    g = torch.Generator().manual_seed(7)
    r = lambda *s, k=1.: (torch.randn(*s, generator=g) * k).cuda()
    q, k, v, vres, gate, mix, gamma = r(G, S, hd), r(G, S, hd), r(G, S, hd), r(G, S, hd), r(G, S, H), r(G, S, H), r(hd, k=.2)
    outs = [torch.empty(G, S, hd, device='cuda') for _ in range(2)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _lib.ptr

    def call(fn, out):
        _lib.check(fn(P(q), S * hd, hd, P(k), S * hd, hd, P(v), S * hd, hd, P(gate), S * H, H, P(gamma), P(vres), S * hd, hd, P(mix), S * H, H, P(out), S * hd, hd,
                      None, G, H, S, S, 50., 1, 1, 0, 0, 1, dh, stream))
    arms = []
    if S <= 160 and (dh == 64 or S <= 64):
        arms.append(lambda: call(lib.d4_small_attn, outs[0]))
    arms.append(lambda: call(lib.d4_small_attn_wide, outs[1]))
    assert lib.d4_debug_switch(b'small_attn_wide', int(forced)) == 0
    res, reps = median_ms(arms)
    new_form = lib.d4_debug_last_form(b'wide_attn').decode()
    out = dict(case=f'self attention {G}x{S}, 8 x {dh} heads', S=S, dh=dh, rows=G * S, reps=reps, new_form=new_form, new_ms=round(res[-1][0], 4),
               new_ms_min=round(res[-1][1], 4), new_ms_max=round(res[-1][2], 4), new_us_per_row=round(1e3 * res[-1][0] / (G * S), 5))
    if len(arms) == 2:
        diff = (outs[0] - outs[1]).abs().max().item() / outs[0].abs().max().item()
        assert diff < 1e-5, diff
        out.update(old_form=lib.d4_debug_last_form(b'small_attn').decode(), old_ms=round(res[0][0], 4), old_ms_min=round(res[0][1], 4), old_ms_max=round(res[0][2], 4),
                   rel_diff=float(f'{diff:.2e}'))
    return out


def step_case(spatial):
    import torch
    import bench
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    cfg = dict(bench.CFG2, num_spatial_tokens=spatial)
    tokens = 1 + spatial + cfg['num_register_tokens'] + 1 + 1
    B, frames = max(1, (bench.B_LOCAL * 15) // tokens), 8
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**cfg, wide_frames=tokens > 64), seed=0, terminal_bias=-10.).cuda()
    gk = dict(return_for_policy_optimization=True, num_steps=bench.NUM_STEPS)
    last = []

    def run():
        last[:] = [m.generate(frames, batch_size=B, **gk)]
    (res,), reps = median_ms([run], windows=7, warm=2, window_s=0.3)
    e = last[0]
    assert e.latents.shape[1] == frames and torch.isfinite(e.latents).all() and torch.isfinite(e.values).all()
    rows = B * tokens
    return dict(case=f'generate {B} x {frames} frames, {tokens} tokens per frame', tokens=tokens, batch=B, rows_per_step=rows, reps=reps, ms_per_step=round(res[0] / frames, 3),
                ms_per_step_min=round(res[1] / frames, 3), ms_per_step_max=round(res[2] / frames, 3), us_per_row=round(1e3 * res[0] / frames / rows, 4))


def child(kind, a, b, c):
    r = attn_case(a, b, c) if kind == 'attn' else step_case(a)
    print(json.dumps(r), flush=True)


def main():
    cases = [('attn', 128, 64, 0), ('attn', 160, 64, 0), ('attn', 64, 64, 1), ('attn', 64, 16, 1), ('attn', 256, 64, 0), ('attn', 512, 64, 0), ('attn', 1024, 64, 0),
             ('step', 4, 0, 0), ('step', 64, 0, 0), ('step', 256, 0, 0)]
    lines, got = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/infer_frame_width.py on an MI355X: median of 7 windows after warm-up (min .. max of the windows alongside); old = d4_small_attn, new = d4_small_attn_wide')
    for kind, a, b, c in cases:
        p = subprocess.run(['timeout', '-k', '10', '150', sys.executable, os.path.abspath(__file__), kind, str(a), str(b), str(c)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} {a} {b} {c}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        say('  '.join(f'{k}={v}' for k, v in r.items()))
    at = {(r['S'], r['dh']): r for r in got if 'S' in r}
    for S in (128, 160):
        r = at[(S, 64)]
        ratio = r['new_ms'] / r['old_ms']
        say(f"(a) {S} tokens per frame: {r['new_form']} {r['new_ms']} ms vs {r['old_form']} {r['old_ms']} ms = {ratio:.3f}x  (expectation: <= 1.10x: {'met' if ratio <= 1.1 else 'NOT met'})")
    for dh in (64, 16):
        r = at[(64, dh)]
        say(f"(b) 64 tokens per frame, head dim {dh}: forced {r['new_form']} {r['new_ms']} ms vs {r['old_form']} {r['old_ms']} ms = {r['new_ms'] / r['old_ms']:.3f}x  (recorded only)")
    base = at[(64, 64)]['new_us_per_row']
    for S in (256, 512, 1024):
        ratio, bound = at[(S, 64)]['new_us_per_row'] / base, S / 64.
        say(f"(c) {S} tokens per frame: time per token row {ratio:.3f}x the forced 64-token figure  (bound: <= {bound:.0f}x: {'met' if ratio <= bound else 'NOT met'})")
    for r in got:
        if 'tokens' in r:
            say(f"(d) {r['case']}: {r['ms_per_step']} ms per imagined step, {r['rows_per_step']} token rows per step = {r['us_per_row']} us per token row  (recorded only)")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'wide_frames_inference.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 5:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        sys.exit(main())
