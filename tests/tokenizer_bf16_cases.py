"""Shared table of the bf16 tokenizer tests (tests/test_tokenizer_bf16_host.py, tests/test_gpu_tokenizer_bf16.py): the cases, their weights and inputs,
the fp32 oracle results and the oracle's own bf16 envelope — computed once per process from oracle/restate.py and tests/bf16_emulation.py alone.
Nothing here reads the code under test beyond constructing a VideoTokenizer for its parameter names and initial values.

E_max of a case = how far restate.tokenizer_decode / tokenizer_tokenize move from their fp32 result when every Linear rounds its operands to bf16, the
maximum over bf16_emulation's four variants, per output and per metric (scaled_max, rel_l2).  The bound of the engine under test is 3 E_max + 1e-4:
the factor of bf16_emulation.check_model and the tolerance of test_gpu_decode.close."""
import functools

import torch

import bf16_emulation as emu
from dreamer4_amd import VideoTokenizer
from oracle import restate

FP32_TOL = 1e-4                       # test_gpu_decode.close
METRICS = dict(scaled_max=emu.scaled_max, rel_l2=emu.rel_l2)

_AC = dict(dim=64, dim_latent=16, patch_size=4, attn_heads=2, time_block_every=2)
CASES = {
    # 64 patches + 32 latents, depth 4: every hand-off on images (K = 64, 128, 192, 256)
    'A': dict(kw=dict(_AC, image_size=32, num_latent_tokens=32, encoder_depth=4, decoder_depth=4), B=2, T=4),
    # dim 96: K = 96 is no multiple of 64 (fp32-activation bf16 kernel) while the head width 128 is: image and fp32-buffer hand-offs mix in one pass
    'B': dict(kw=dict(dim=96, dim_latent=8, patch_size=4, attn_heads=2, time_block_every=2, image_height=16, image_width=24, num_latent_tokens=6,
                      encoder_depth=2, decoder_depth=2), B=2, T=4),
    # 96 patches + 8 latents: the route for 65 .. 160 tokens per frame without wide_frames
    'C': dict(kw=dict(_AC, dim_latent=8, image_height=32, image_width=48, num_latent_tokens=8, encoder_depth=2, decoder_depth=2), B=2, T=4),
    # 256 patches + 16 latents: the tiled wide core
    'D': dict(kw=dict(_AC, dim_latent=8, image_size=64, num_latent_tokens=16, encoder_depth=2, decoder_depth=2, wide_frames=True), B=1, T=2),
}
CASES['E'] = dict(CASES['D'], kw=dict(CASES['D']['kw'], attn_products='bf16'), oracle_of='D')      # the oracle has no attention-product option


def fresh(kw, seed=0, **extra):
    """test_gpu_decode._fresh, with the learned latent tokens scaled as test_tokenize_vs_oracle_on_fresh_weights scales them."""
    torch.manual_seed(seed)
    tok = VideoTokenizer(**kw, **extra)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in tok.named_parameters():
            if p.ndim == 1 and ('norm' in k or k.endswith('.0.weight')):
                p.copy_(1. + torch.randn(p.shape, generator=g) * 0.1)
            elif k.endswith('gamma'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
        tok.latent_tokens.mul_(30.)
    return tok


def oracle_config(kw):
    args = {k: v for k, v in kw.items() if k not in ('image_size', 'wide_frames', 'attn_products', 'matmul_dtype')}
    if 'image_size' in kw:
        args['image_height'] = args['image_width'] = kw['image_size']
    return restate.TokenizerConfig(**args)


def envelope(run, ref):
    """{output: {metric: E_max}} of run(nudge) -> {output: tensor} against the fp32 results `ref`."""
    outs = emu.run_variants(run)
    return {k: {m: max(f(o[k], ref[k]) for o in outs) for m, f in METRICS.items()} for k in ref}


def oracle_runner(tc, W, lat, noise, video):
    def run(nudge):
        s = 1. + nudge
        Wn = {k: (v * s if v.is_floating_point() and not k.endswith('inv_freq') else v) for k, v in W.items()}
        return dict(decode=restate.tokenizer_decode(tc, Wn, lat * s, noise * s), tokenize=restate.tokenizer_tokenize(tc, Wn, video * s))
    return run


@functools.lru_cache(maxsize=None)
def reference(name):
    """Weights, inputs, fp32 oracle results and E_max of a case (cases that name `oracle_of` share that case's)."""
    case = CASES[name]
    if 'oracle_of' in case:
        return reference(case['oracle_of'])
    kw, B, T = case['kw'], case['B'], case['T']
    tok = fresh(kw)
    W = {k: v.detach().clone() for k, v in tok.state_dict().items()}
    tc = oracle_config(kw)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, T, kw['num_latent_tokens'], kw['dim_latent'], generator=g).clamp(-1, 1)
    noise = torch.randn(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    video = torch.rand(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    run = oracle_runner(tc, W, lat, noise, video)
    with torch.no_grad():
        ref = {k: v.clone() for k, v in run(0.).items()}
        E = envelope(run, ref)
    return dict(tc=tc, W=W, lat=lat, noise=noise, video=video, ref=ref, E=E, run=run)


def bound(E):
    return 3. * E + FP32_TOL


def build(name, **extra):
    """The case's tokenizer (fresh weights; `extra` e.g. matmul_dtype='bf16')."""
    return fresh(CASES[name]['kw'], **extra)
