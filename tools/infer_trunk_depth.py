"""Deep trunks in inference: what the chunked AttentionPool mix (csrc/pool_mix_deep.hip) costs.
    python tools/infer_trunk_depth.py            (on an MI355X; the output is profiles/deep_trunk_inference.txt)
(a) like for like: the pool mix at D 512 x 3840 token rows and D 1024 x 1792 token rows, fp32 and bf16 keys: pool_mix at L = 64 (the yardstick,
    the unchanged kernel in the same build) against pool_mix_deep at L = 65, 129, 257, time per (row . hidden); and pool_mix_deep at L = 64
(b) few rows: 11 token rows at D 512, pool_mix at L = 64 against pool_mix_deep at L = 65, 129, time per hidden
(c) the path not taken, at L = 129, 3840 rows, D 512: key GEMM (L M x 256) + pool_mix_deep + per-head value GEMM against the key-and-value
    GEMM (L M x 512) + d4_small_attn_wide with one query per row
(d) generate() with config 2's architecture (bench.py CFG2: dim 512, 8 x 64 heads, 15 tokens per frame) at B 64, 8 frames, depth 31
    (wide_frames=False) and depth 32 / 48 (wide_frames=True): ms per imagined step, us per token row per layer
Timing: the arms of a comparison in one process, their windows alternating; 3 warm-up runs, then 7 windows of `reps` runs each between
device synchronisations (reps calibrated on the first arm to ~0.1 s per window); the figure is the median window.  Every case is a process
of its own under `timeout`; the first failure ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
EPS = 1.1920929e-07
RMS_ROWSCALE = 1                                            # csrc/kernels.h: GEMM_RMS_ROWSCALE


def _operands(D, M, L, kb):
    import torch
    g = torch.Generator(device='cuda').manual_seed(7)
    r = lambda *s, k=1.: torch.randn(*s, generator=g, device='cuda') * k
    d = dict(q=r(M, 256), k=r(L, M, 256), hid=r(L, M, D), gw=r(4, D, k=2 * D ** -0.5), gamma=r(4, 64, k=.2))
    if kb:
        d['k_b'] = d['k'].to(torch.bfloat16)
        d['hid_b'] = d['hid'].to(torch.bfloat16)
    return d


def _mix_call(lib, fn, d, D, M, L, u, kb):
    """one pool over the first L hiddens of the operands (in-loop pool: x is hidden L - 1), as the engine calls it"""
    from dreamer4_amd import _lib
    P = _lib.ptr
    stream = C.c_void_p(__import__('torch').cuda.current_stream().cuda_stream)
    xp = C.c_void_p(d['hid'].data_ptr() + 4 * (L - 1) * M * D)
    hid_b = P(d['hid_b']) if kb and D > 512 else None          # (engine: the bf16 hidden image where the wave-per-row form is certain)
    return lambda: _lib.check(fn(P(d['q']), 256, xp, D, P(d['gw']), None if kb else P(d['k']), 256, P(d['hid']), D, P(d['gamma']), P(u), M, L, 4, EPS,
                                 None, P(d['k_b']) if kb else None, None, hid_b, stream))


def mix_case(D, M, kb):
    """arm 0: d4_pool_mix at L = 64; then d4_pool_mix_deep at L = 64 and at each deep L"""
    import torch
    from infer_frame_width import median_ms
    from dreamer4_amd import _lib
    lib = _lib.load()
    deep_L = (65, 129, 257) if M > 64 else (65, 129)
    d = _operands(D, M, max(deep_L), kb)
    us = [torch.empty(M, 4, D, device='cuda') for _ in range(2 + len(deep_L))]
    arms = [_mix_call(lib, lib.d4_pool_mix, d, D, M, 64, us[0], kb), _mix_call(lib, lib.d4_pool_mix_deep, d, D, M, 64, us[1], kb)]
    arms += [_mix_call(lib, lib.d4_pool_mix_deep, d, D, M, L, us[2 + i], kb) for i, L in enumerate(deep_L)]
    res, reps = median_ms(arms)
    diff = ((us[0] - us[1]).abs().max() / us[0].abs().max()).item()
    assert diff < 1e-5 and all(torch.isfinite(u).all() for u in us), diff
    out = dict(case=f'pool mix D {D} x {M} rows, ' + ('bf16' if kb else 'fp32') + ' keys', D=D, M=M, kb=kb, reps=reps, old_form=lib.d4_debug_last_form(b'pool_mix').decode(),
               new_form=lib.d4_debug_last_form(b'pool_mix_deep').decode(), rel_diff_at_64=float(f'{diff:.2e}'))
    for name, L, (med, lo, hi) in [('old64', 64, res[0]), ('new64', 64, res[1])] + [(f'new{L}', L, res[2 + i]) for i, L in enumerate(deep_L)]:
        out.update({f'{name}_ms': round(med, 4), f'{name}_ms_min': round(lo, 4), f'{name}_ms_max': round(hi, 4), f'{name}_ns_per_row_hidden': round(1e6 * med / (M * L), 4)})
    return out


def path_case(D, M, L):
    """the two ways through a pool at L hiddens, projections included (fp32 engine)"""
    import torch
    from infer_frame_width import median_ms
    from dreamer4_amd import _lib
    lib = _lib.load()
    P = _lib.ptr
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = _operands(D, M, L, 0)
    g = torch.Generator(device='cuda').manual_seed(9)
    Wkv = torch.randn(512, D, generator=g, device='cuda') * D ** -0.5          # [keys 256 | values 256] x D
    keys, kv = torch.empty(L * M, 256, device='cuda'), torch.empty(L * M, 512, device='cuda')
    u, att_a, att_b = torch.empty(M, 4, D, device='cuda'), torch.empty(M, 256, device='cuda'), torch.empty(M, 256, device='cuda')
    gate = torch.randn(M, 4, generator=g, device='cuda')
    xp = C.c_void_p(d['hid'].data_ptr() + 4 * (L - 1) * M * D)

    def mix_path():
        _lib.check(lib.d4_gemm(P(d['hid']), D, P(Wkv), D, P(keys), 256, None, None, 0, L * M, 256, D, RMS_ROWSCALE, EPS, stream))
        _lib.check(lib.d4_pool_mix_deep(P(d['q']), 256, xp, D, P(d['gw']), P(keys), 256, P(d['hid']), D, P(d['gamma']), P(u), M, L, 4, EPS, None, None, None, None, stream))
        _lib.check(lib.d4_gemm_batched(P(u), 4 * D, C.c_void_p(Wkv.data_ptr() + 4 * 256 * D), D, P(att_a), 256, None, None, 0, M, 64, D, 0, EPS, 4, D, 64 * D, 64, stream))

    def kv_path():
        _lib.check(lib.d4_gemm(P(d['hid']), D, P(Wkv), D, P(kv), 512, None, None, 0, L * M, 512, D, RMS_ROWSCALE, EPS, stream))
        _lib.check(lib.d4_small_attn_wide(P(d['q']), 256, 0, P(kv), 512, M * 512, C.c_void_p(kv.data_ptr() + 4 * 256), 512, M * 512, P(gate), 4, 0, P(d['gamma']),
                                          None, 0, 0, None, 0, 0, P(att_b), 256, 0, None, M, 4, 1, L, 0., 0, 0, 0, 0, 1, 64, stream))
    res, reps = median_ms([mix_path, kv_path])
    assert torch.isfinite(att_a).all() and torch.isfinite(att_b).all()
    return dict(case=f'one pool over {L} hiddens, {M} rows, D {D}', L=L, reps=reps, mix_path_ms=round(res[0][0], 4), mix_path_ms_min=round(res[0][1], 4),
                mix_path_ms_max=round(res[0][2], 4), kv_path_ms=round(res[1][0], 4), kv_path_ms_min=round(res[1][1], 4), kv_path_ms_max=round(res[1][2], 4),
                kv_form=lib.d4_debug_last_form(b'wide_attn').decode())


def step_case(depth):
    import torch
    import bench
    from infer_frame_width import median_ms
    from dreamer4_amd import DynamicsWorldModel
    from dreamer4_amd.synthetic import randomize_weights
    cfg = dict(bench.CFG2, depth=depth)
    tokens = 1 + cfg['num_spatial_tokens'] + cfg['num_register_tokens'] + 1 + 1
    B, frames = 64, 8
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(**cfg, wide_frames=2 * depth + 1 > 64), seed=0, terminal_bias=-10.).cuda()
    gk = dict(return_for_policy_optimization=True, num_steps=bench.NUM_STEPS)
    last = []

    def run():
        last[:] = [m.generate(frames, batch_size=B, **gk)]
    (res,), reps = median_ms([run], windows=7, warm=2, window_s=0.3)
    e = last[0]
    assert e.latents.shape[1] == frames and torch.isfinite(e.latents).all() and torch.isfinite(e.values).all()
    rows = B * tokens
    return dict(case=f'generate {B} x {frames} frames, {tokens} tokens per frame, depth {depth}', depth=depth, rows_per_step=rows, reps=reps, ms_per_step=round(res[0] / frames, 3),
                ms_per_step_min=round(res[1] / frames, 3), ms_per_step_max=round(res[2] / frames, 3), us_per_row_per_layer=round(1e3 * res[0] / frames / rows / depth, 4))


def child(kind, a, b, c):
    r = mix_case(a, b, c) if kind == 'mix' else path_case(a, b, c) if kind == 'path' else step_case(a)
    print(json.dumps(r), flush=True)


def main():
    cases = [('mix', 512, 3840, 0), ('mix', 512, 3840, 1), ('mix', 1024, 1792, 0), ('mix', 1024, 1792, 1), ('mix', 512, 11, 0), ('path', 512, 3840, 129),
             ('step', 31, 0, 0), ('step', 32, 0, 0), ('step', 48, 0, 0)]
    lines, got = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/infer_trunk_depth.py on an MI355X: median of 7 windows after warm-up (min .. max of the windows alongside); old = d4_pool_mix at L = 64, new = d4_pool_mix_deep')
    for kind, a, b, c in cases:
        p = subprocess.run(['timeout', '-k', '10', '200', sys.executable, os.path.abspath(__file__), kind, str(a), str(b), str(c)], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'{kind} {a} {b} {c}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        got.append(r)
        say('  '.join(f'{k}={v}' for k, v in r.items()))
    for r in got:
        if 'old64_ms' not in r:
            continue
        tag, unit = ('(a)', 'per (row . hidden)') if r['M'] > 64 else ('(b)', 'per hidden')
        base = r['old64_ns_per_row_hidden']
        for L in (65, 129, 257):
            if f'new{L}_ms' in r:
                ratio = r[f'new{L}_ns_per_row_hidden'] / base
                say(f"{tag} {r['case']}, L = {L}: {r['new_form']} {r[f'new{L}_ms']} ms vs {r['old_form']} at L = 64 {r['old64_ms']} ms: time {unit} {ratio:.3f}x  "
                    f"(expectation: <= 1.10x: {'met' if ratio <= 1.1 else 'missed'})")
        say(f"{tag} {r['case']}, L = 64: forced {r['new_form']} {r['new64_ms']} ms vs {r['old_form']} {r['old64_ms']} ms = {r['new64_ms'] / r['old64_ms']:.3f}x  (recorded only)")
    for r in got:
        if 'mix_path_ms' in r:
            say(f"(c) {r['case']}: key GEMM + pool_mix_deep + value GEMM {r['mix_path_ms']} ms vs key-and-value GEMM + {r['kv_form']} {r['kv_path_ms']} ms = "
                f"{r['mix_path_ms'] / r['kv_path_ms']:.3f}x  (recorded only)")
    for r in got:
        if 'depth' in r:
            say(f"(d) {r['case']}: {r['ms_per_step']} ms per imagined step, {r['us_per_row_per_layer']} us per token row per layer  (recorded only)")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'deep_trunk_inference.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 5:
        child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        sys.exit(main())
