"""VideoTokenizer(matmul_dtype='bf16') against the default fp32 tokenizer: time per decode / tokenize call, the end projections' share, workspace.
    python tools/tokenizer_bf16.py            (on an MI355X; the output is profiles/tokenizer_bf16.txt)
Shapes: dim 512, 8 heads of 64, encoder and decoder depth 4, time_block_every 4, patch 4, dim_latent 32, 8 clips of 16 frames, at
    (a) 128 patches + 32 latents per frame (32 x 64 image; attn_wide_kernel)          (b) 256 patches + 64 latents (64 x 64 image; wide_frames=True, the tiled core)
Both tokenizers hold the same weights and live in one process; the arms' windows alternate (tools/infer_frame_width.py median_ms: 3 warm-up calls, then 7
windows of `reps` calls between device synchronisations, reps calibrated to ~0.3 s per window; the figure is the median window, min .. max alongside).
The end projections (patch rows -> tokens + LayerNorm, latents -> decoder tokens, tokens -> patch rows; patch rows -> tokens + LayerNorm, latent tokens ->
latents + tanh) stay fp32 in both modes: they are timed as operators of their own at the call's shapes (d4_gemm, d4_layernorm_rows, d4_unary_rows), and the
share is that time over the call's.  Every shape is a process of its own under `timeout`; the first failure ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SHAPES = {'a': dict(image_height=32, image_width=64, num_latent_tokens=32, wide_frames=False),
          'b': dict(image_height=64, image_width=64, num_latent_tokens=64, wide_frames=True)}
B, T = 8, 16


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def child(shape):
    import torch
    from infer_frame_width import median_ms
    from dreamer4_amd import VideoTokenizer, _lib
    lib = _lib.load()
    kw = dict(dim=512, dim_latent=32, patch_size=4, attn_heads=8, encoder_depth=4, decoder_depth=4, time_block_every=4, **SHAPES[shape])
    torch.manual_seed(0)
    f32 = VideoTokenizer(**kw)
    with torch.no_grad():
        f32.latent_tokens.mul_(30.)
    b16 = VideoTokenizer(**kw, matmul_dtype='bf16')
    b16.load_state_dict(f32.state_dict())
    f32, b16 = f32.cuda(), b16.cuda()
    g = torch.Generator().manual_seed(1)
    H, W, n, dl, D = kw['image_height'], kw['image_width'], kw['num_latent_tokens'], kw['dim_latent'], kw['dim']
    lat = torch.randn(B, T, n, dl, generator=g).clamp(-1, 1).cuda()
    noise = torch.randn(B, 3, T, H, W, generator=g).cuda()
    video = torch.rand(B, 3, T, H, W, generator=g).cuda()
    out = dict(shape=shape, patches=(H // 4) * (W // 4), latents=n, frames=B * T)
    keep = {}

    def arm(tok, what):
        if what == 'decode':
            return lambda: keep.__setitem__((tok.matmul_dtype, what), tok.decode(lat, noise=noise))
        return lambda: keep.__setitem__((tok.matmul_dtype, what), tok.tokenize(video))
    for what in ('decode', 'tokenize'):
        (r32, r16), reps = median_ms([arm(f32, what), arm(b16, what)], windows=7, warm=3, window_s=0.3)
        a, b = keep[('fp32', what)], keep[('bf16', what)]
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)
        out[what] = dict(reps=reps, fp32_ms=[round(x, 4) for x in r32], bf16_ms=[round(x, 4) for x in r16], rel_l2_bf16_vs_fp32=float(f'{rel_l2(b, a):.3e}'))
    # the end projections as operators of their own, at the calls' shapes
    P_, dp, Fr = out['patches'], 48, B * T
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    pt = _lib.ptr

    def gemm(A, Wt, Cm, bias, M, N, K, flags=0):
        return lambda: _lib.check(lib.d4_gemm(pt(A), K, pt(Wt), K, pt(Cm), N, pt(bias) if bias is not None else None, None, 0, M, N, K, flags, 1.1920928955078125e-07, stream))
    rows, tokD, lrows, ltok, lz = r(Fr * P_, dp), torch.empty(Fr * P_, D, device='cuda'), r(Fr * n, dl), torch.empty(Fr * n, D, device='cuda'), torch.empty(Fr * n, dl, device='cuda')
    w_in, b_in, ln, w_lat, b_lat, w_out, b_out, w_z = r(D, dp), r(D), r(D), r(D, dl), r(D), r(dp, D), r(dp), r(dl, D)
    back = torch.empty(Fr * P_, dp, device='cuda')
    layernorm = lambda: _lib.check(lib.d4_layernorm_rows(pt(tokD), D, pt(ln), None, pt(tokD), D, Fr * P_, D, 1e-5, 0, stream))
    tanh = lambda: _lib.check(lib.d4_unary_rows(1, pt(lz), pt(lz), lz.numel(), stream))
    g_in, g_lat, g_out, g_z = (gemm(rows, w_in, tokD, b_in, Fr * P_, D, dp), gemm(lrows, w_lat, ltok, b_lat, Fr * n, D, dl),
                               gemm(tokD, w_out, back, b_out, Fr * P_, dp, D, _lib.GEMM_RMS_ROWSCALE), gemm(ltok, w_z, lz, None, Fr * n, dl, D, _lib.GEMM_RMS_ROWSCALE))

    def decode_ends():
        g_in(); layernorm(); g_lat(); g_out()

    def tokenize_ends():
        g_in(); layernorm(); g_z(); tanh()
    (rd, rt), _ = median_ms([decode_ends, tokenize_ends], windows=7, warm=3, window_s=0.1)
    out['decode']['ends_ms'], out['tokenize']['ends_ms'] = [round(x, 4) for x in rd], [round(x, 4) for x in rt]
    out['workspace_bytes'] = {tok.matmul_dtype: {('decoder', 'encoder')[mode - 1]: int(lib.d4_engine_workspace_bytes(tok._engines[mode]['engine'])) for mode in (1, 2)}
                              for tok in (f32, b16)}
    print(json.dumps(out), flush=True)


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('# tools/tokenizer_bf16.py on an MI355X: dim 512, 8 x 64 heads, depth 4 + 4, 8 x 16 frames; ms per call = median of 7 alternating windows (min .. max)')
    for shape in SHAPES:
        p = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), shape], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print(f'shape {shape}: FAILED with exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}', flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        say(f"({shape}) {r['patches']} patches + {r['latents']} latents per frame, {r['frames']} frames" + (', wide_frames=True' if SHAPES[shape]['wide_frames'] else ''))
        for what in ('decode', 'tokenize'):
            d = r[what]
            f, b, e = d['fp32_ms'], d['bf16_ms'], d['ends_ms']
            beats = b[2] < f[1]
            say(f"    {what:8s} fp32 {f[0]:.3f} ms ({f[1]:.3f} .. {f[2]:.3f})   bf16 {b[0]:.3f} ms ({b[1]:.3f} .. {b[2]:.3f})   bf16 / fp32 = {b[0] / f[0]:.3f}   "
                f"bf16's slowest window {'beats' if beats else 'does NOT beat'} fp32's fastest   ({d['reps']} calls per window)")
            say(f"    {what:8s} end projections alone (fp32 in both modes): {e[0]:.3f} ms ({e[1]:.3f} .. {e[2]:.3f}) = {100 * e[0] / f[0]:.1f} % of the fp32 call, "
                f"{100 * e[0] / b[0]:.1f} % of the bf16 call;   rel l2 of the bf16 result against the fp32 one {d['rel_l2_bf16_vs_fp32']:.3e}")
        w = r['workspace_bytes']
        for part in ('decoder', 'encoder'):
            say(f"    workspace {part}: fp32 {w['fp32'][part] / 2 ** 20:.1f} MiB   bf16 {w['bf16'][part] / 2 ** 20:.1f} MiB   (+{100 * (w['bf16'][part] / w['fp32'][part] - 1):.1f} %)")
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'tokenizer_bf16.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 2:
        child(sys.argv[1])
    else:
        sys.exit(main())
