"""Wide frames in inference: what the bf16-product form of the wide attention core (csrc/attn_wide_bf16.hip) buys.
    python tools/infer_attn_bf16.py            (on an MI355X; the output is profiles/wide_attn_bf16.txt)
(a) self attention with belief projection and value residual (8 x 64 heads) at 256, 512 and 1024 tokens per frame (3840 / 3584 / 3072 token
    rows): wide_attn_kernel<64> through d4_small_attn_wide (unchanged by this option: it stands for the fp32 products) against
    wide_attn_bf16_kernel<64> through d4_small_attn_wide_bf16; absolute times and the TFLOP/s of the two products (4 S^2 dh per head and frame)
(b) the same at 256 tokens per frame, head dims 32 and 16 (recorded only)
(c) generate() with config 5's architecture (bench.py CFG5, matmul_dtype='bf16') and with config 2's (fp32) at num_spatial_tokens=256,
    wide_frames=True, attn_products 'fp32' against 'bf16', the batch chosen so that the token rows per step match the configuration's own
    (recorded only)
Timing: both arms of a comparison in one process, their windows alternating; warm-up runs, then 7 windows of `reps` runs each between
device synchronisations; the figure is the median window.  Every case is a process of its own under `timeout`; the first failure ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from infer_frame_width import ROWS, median_ms  # noqa: E402


def attn_case(S, dh):
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
    res, reps = median_ms([lambda: call(lib.d4_small_attn_wide, outs[0]), lambda: call(lib.d4_small_attn_wide_bf16, outs[1])])
    diff = (outs[0] - outs[1]).abs().max().item() / outs[0].abs().max().item()
    assert 0. < diff < 3e-2, diff
    flop = 4. * G * H * S * S * dh
    rd = lambda x: round(x, 4)
    return dict(case=f'self attention {G}x{S}, 8 x {dh} heads', S=S, dh=dh, rows=G * S, reps=reps, fp32_form=lib.d4_debug_last_form(b'wide_attn').decode(),
                fp32_ms=rd(res[0][0]), fp32_ms_min=rd(res[0][1]), fp32_ms_max=rd(res[0][2]), fp32_tflops=round(flop / res[0][0] / 1e9, 1),
                bf16_form=lib.d4_debug_last_form(b'wide_attn_bf16').decode(), bf16_ms=rd(res[1][0]), bf16_ms_min=rd(res[1][1]), bf16_ms_max=rd(res[1][2]),
                bf16_tflops=round(flop / res[1][0] / 1e9, 1), rel_diff=float(f'{diff:.2e}'))


def step_case(which):
    import torch
    import bench
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    base, dtype, b_own = (bench.CFG5, 'bf16', 128) if which == 5 else (bench.CFG2, 'fp32', bench.B_LOCAL)
    cfg = dict(base, num_spatial_tokens=256, matmul_dtype=dtype, wide_frames=True)
    probe = DynamicsWorldModel(**dict(base, matmul_dtype=dtype))
    extra = 2 + probe.num_register_tokens + (1 if (base.get('num_discrete_actions') or base.get('num_continuous_actions')) else 0)
    own_tokens, tokens = extra + probe.num_spatial_tokens, extra + 256
    del probe
    B, frames = max(1, (b_own * own_tokens) // tokens), 4
    ms, last = [], [None, None]
    for prod in ('fp32', 'bf16'):
        torch.manual_seed(0)
        ms.append(randomize_weights(DynamicsWorldModel(**cfg, attn_products=prod), seed=0, terminal_bias=-10.).cuda())
    gk = dict(return_for_policy_optimization=True, num_steps=bench.NUM_STEPS)

    def arm(i):
        def run():
            last[i] = ms[i].generate(frames, batch_size=B, **gk)
        return run
    res, reps = median_ms([arm(0), arm(1)], windows=7, warm=2, window_s=0.3)
    for e in last:
        assert e.latents.shape[1] == frames and torch.isfinite(e.latents).all() and torch.isfinite(e.values).all()
    rd = lambda x: round(x / frames, 3)
    return dict(case=f"generate {B} x {frames} frames, config {which}'s architecture, matmul_dtype={dtype}, {tokens} tokens per frame", config=which, batch=B,
                rows_per_step=B * tokens, reps=reps, fp32_ms_per_step=rd(res[0][0]), fp32_ms_per_step_min=rd(res[0][1]), fp32_ms_per_step_max=rd(res[0][2]),
                bf16_ms_per_step=rd(res[1][0]), bf16_ms_per_step_min=rd(res[1][1]), bf16_ms_per_step_max=rd(res[1][2]))


def child(kind, a, b):
    r = attn_case(a, b) if kind == 'attn' else step_case(a)
    print(json.dumps(r), flush=True)


def main():
    cases = [('attn', 256, 64), ('attn', 512, 64), ('attn', 1024, 64), ('attn', 256, 32), ('attn', 256, 16), ('step', 5, 0), ('step', 2, 0)]
    lines, got = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/infer_attn_bf16.py on an MI355X: median of 7 windows after warm-up (min .. max of the windows alongside); fp32 = d4_small_attn_wide / '
        "attn_products='fp32', bf16 = d4_small_attn_wide_bf16 / attn_products='bf16'")
    for kind, a, b in cases:
        p = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), kind, str(a), str(b)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} {a} {b}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        say('  '.join(f'{k}={v}' for k, v in r.items()))
    for r in got:
        if 'S' not in r:
            continue
        ratio = r['bf16_ms'] / r['fp32_ms']
        if r['dh'] == 64:
            note = f"required: < 1.0x: {'met' if ratio < 1. else 'NOT met'}"
            if r['S'] == 1024:
                note += f"; expected: <= 0.5x: {'met' if ratio <= .5 else 'NOT met'}"
            tag = '(a)'
        else:
            note, tag = 'recorded only', '(b)'
        say(f"{tag} {r['S']} tokens per frame, head dim {r['dh']}: {r['bf16_form']} {r['bf16_ms']} ms ({r['bf16_tflops']} TFLOP/s in the two products) vs {r['fp32_form']} "
            f"{r['fp32_ms']} ms ({r['fp32_tflops']} TFLOP/s) = {ratio:.3f}x  ({note})")
    for r in got:
        if 'config' in r:
            say(f"(c) {r['case']}: attn_products='bf16' {r['bf16_ms_per_step']} ms per imagined step vs 'fp32' {r['fp32_ms_per_step']} ms = "
                f"{r['bf16_ms_per_step'] / r['fp32_ms_per_step']:.3f}x  (recorded only)")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'wide_attn_bf16.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
