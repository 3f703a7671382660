"""GPU: VideoTokenizer(matmul_dtype='bf16') — decode and tokenize with the trunks' Linears on the bf16 matrix pipe.

The yardstick is the oracle's own bf16 envelope (tests/tokenizer_bf16_cases.py, tests/bf16_emulation.py): the engine may sit at most 3 E_max + 1e-4
from the fp32 oracle in scaled_max and in rel_l2.  Every figure is printed before it is asserted."""
import ctypes as C

import pytest
import torch

import tokenizer_bf16_cases as cases
from dreamer4_amd import DynamicsWorldModel, _lib
from oracle import restate
from util import make_noise, oracle_config, randomize_weights

pytestmark = pytest.mark.gpu


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_both(tok, R):
    tok = tok.cuda()
    return dict(decode=tok.decode(R['lat'], noise=R['noise']).cpu(), tokenize=tok.tokenize(R['video']).cpu())


_FP32 = {}


def fp32_engine(name):
    """decode / tokenize of the case on the default (fp32) engine, once per process."""
    if name not in _FP32:
        _FP32[name] = run_both(cases.build(name), cases.reference(name))
    return _FP32[name]


def check_envelope(got, R, slack=None, label=''):
    bad = []
    for out in ('decode', 'tokenize'):
        for metric, f in cases.METRICS.items():
            d, b = f(got[out], R['ref'][out]), cases.bound(R['E'][out][metric]) + (slack[out][metric] if slack else 0.)
            print(f'{label}{out} {metric}: {d:.3e}  E_max {R["E"][out][metric]:.3e}  bound {b:.3e}')
            if not d <= b:
                bad.append((out, metric, d, b))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 1. envelope
@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_bf16_engine_within_the_oracles_envelope(name):
    R = cases.reference(name)
    got = run_both(cases.build(name, matmul_dtype='bf16'), R)
    f32 = fp32_engine(name)
    check_envelope(got, R, label=f'case {name} ')
    for out in got:
        assert torch.isfinite(got[out]).all()
        assert not torch.equal(got[out], f32[out]), f'{out}: the bf16 engine returned the fp32 engine\'s bits - bf16 did not run'
    assert got['tokenize'].abs().max().item() < 1.


def test_bf16_engine_with_bf16_attention_products():
    """Case E: the bound plus what the existing fp32-GEMM attn_products='bf16' tokenizer (parent behaviour) deviates from the oracle on the same inputs."""
    R = cases.reference('E')
    parent = run_both(cases.build('E'), R)
    slack = {out: {m: f(parent[out], R['ref'][out]) for m, f in cases.METRICS.items()} for out in parent}
    print('attn_products=bf16 with fp32 GEMMs vs the oracle:', slack)
    got = run_both(cases.build('E', matmul_dtype='bf16'), R)
    check_envelope(got, R, slack=slack, label='case E ')
    for out in got:
        assert not torch.equal(got[out], parent[out])


# ------------------------------------------------------------------------------------------------ 2. default path unchanged
@pytest.mark.parametrize('name', ['A', 'D'])
def test_explicit_fp32_is_the_default_path(name):
    R = cases.reference(name)
    lib = _lib.load()
    a, b = cases.build(name), cases.build(name, matmul_dtype='fp32')
    ra, rb = fp32_engine(name), run_both(b, R)
    for out in ra:
        assert torch.equal(ra[out], rb[out]), out
    a = a.cuda()
    a.decode(R['lat'], noise=R['noise']); a.tokenize(R['video'])
    for mode in (1, 2):
        wa, wb = (lib.d4_engine_workspace_bytes(t._engines[mode]['engine']) for t in (a, b))
        assert wa == wb, (mode, wa, wb)
    # ... and the bf16 engines' workspaces are the larger ones (mirrors + images)
    c = cases.build(name, matmul_dtype='bf16').cuda()
    c.decode(R['lat'], noise=R['noise']); c.tokenize(R['video'])
    for mode in (1, 2):
        assert lib.d4_engine_workspace_bytes(c._engines[mode]['engine']) > lib.d4_engine_workspace_bytes(a._engines[mode]['engine'])


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize('name', ['A', 'D'])
def test_bf16_decode_and_tokenize_are_reproducible(name):
    R = cases.reference(name)
    tok = cases.build(name, matmul_dtype='bf16').cuda()
    v1, v2 = tok.decode(R['lat'], noise=R['noise']), tok.decode(R['lat'], noise=R['noise'])
    assert torch.equal(v1, v2)
    z1, z2 = tok.tokenize(R['video']), tok.tokenize(R['video'])
    assert torch.equal(z1, z2)
    other = cases.build(name, matmul_dtype='bf16').cuda()          # a second engine on the same weights
    assert torch.equal(other.decode(R['lat'], noise=R['noise']), v1)


# ------------------------------------------------------------------------------------------------ 4. pack operators
@pytest.mark.parametrize('D', [64, 100, 30])         # 16-byte, 8-byte and element stores of the image
@pytest.mark.parametrize('which', [0, 1], ids=['decoder', 'encoder'])
def test_pack_operator_with_image(which, D):
    lib = _lib.load()
    Fr, P, n_lat, pad = 3, 24, 6, 64
    n_total = n_lat + 1 if which == 0 else n_lat                 # decoder: 6 of 7 latent rows kept; encoder: the 6 learned tokens
    g = torch.Generator().manual_seed(7 + which + D)
    S = P + n_lat
    img = torch.randn(Fr, P, D, generator=g).cuda()
    pos = torch.randn(P, D, generator=g).cuda()
    lat = (torch.randn(Fr, n_total, D, generator=g) if which == 0 else torch.randn(n_lat, D, generator=g)).cuda()
    ncomp = Fr * (P if which == 0 else n_lat) * D

    def bufs():
        return (torch.full((Fr * S * D + pad,), -7., device='cuda'), torch.full((ncomp + pad,), -7., device='cuda'))
    tok0, comp0 = bufs()
    _lib.check(lib.d4_pack_tokens(which, _lib.ptr(tok0), _lib.ptr(comp0), _lib.ptr(pos) if which == 0 else None, _lib.ptr(img), _lib.ptr(lat), Fr, P, n_lat, n_total, D, stream()))
    tok1, comp1 = bufs()
    image = torch.full((Fr * S * D + pad,), 3., device='cuda').to(torch.bfloat16)
    cimage = torch.full((ncomp + pad,), 3., device='cuda').to(torch.bfloat16)
    _lib.check(lib.d4_pack_tokens_bf16(which, _lib.ptr(tok1), _lib.ptr(image), _lib.ptr(comp1), _lib.ptr(cimage), _lib.ptr(pos) if which == 0 else None, _lib.ptr(img),
                                       _lib.ptr(lat), Fr, P, n_lat, n_total, D, stream()))
    # ... and without the compact copy's image
    tok2, comp2 = bufs()
    image2 = torch.full((Fr * S * D + pad,), 3., device='cuda').to(torch.bfloat16)
    _lib.check(lib.d4_pack_tokens_bf16(which, _lib.ptr(tok2), _lib.ptr(image2), _lib.ptr(comp2), None, _lib.ptr(pos) if which == 0 else None, _lib.ptr(img),
                                       _lib.ptr(lat), Fr, P, n_lat, n_total, D, stream()))
    torch.cuda.synchronize()
    assert torch.equal(tok1, tok0) and torch.equal(comp1, comp0)
    assert torch.equal(tok2, tok0) and torch.equal(comp2, comp0) and torch.equal(image2, image)
    rows = tok0[:Fr * S * D]
    assert not (rows == -7.).any() and not (comp0[:ncomp] == -7.).any(), 'every row is written'
    # against the plain definition, too
    t = tok0[:Fr * S * D].view(Fr, S, D)
    if which == 0:
        assert torch.equal(t[:, :P], pos[None] + img) and torch.equal(t[:, P:], lat[:, :n_lat]) and torch.equal(comp0[:ncomp].view(Fr, P, D), t[:, :P])
    else:
        assert torch.equal(t[:, :P], img) and torch.equal(t[:, P:], lat[None].expand(Fr, -1, -1)) and torch.equal(comp0[:ncomp].view(Fr, n_lat, D), t[:, P:])
    assert torch.equal(image[:Fr * S * D], rows.to(torch.bfloat16)), 'the image is the rows rounded to nearest even'
    assert torch.equal(cimage[:ncomp], comp0[:ncomp].to(torch.bfloat16)), 'the compact copy\'s image likewise'
    assert (tok1[Fr * S * D:] == -7.).all() and (comp1[ncomp:] == -7.).all() and (image[Fr * S * D:].float() == 3.).all() and (cimage[ncomp:].float() == 3.).all(), 'padding untouched'


def test_pack_operator_refuses_bad_arguments():
    lib = _lib.load()
    x = torch.zeros(64, device='cuda')
    assert lib.d4_pack_tokens_bf16(0, _lib.ptr(x), None, _lib.ptr(x), None, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 1, 1, 1, 1, 4, stream()) != 0      # no image
    assert lib.d4_pack_tokens_bf16(0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, None, _lib.ptr(x), _lib.ptr(x), 1, 1, 1, 1, 4, stream()) != 0      # decoder without pos
    assert lib.d4_pack_tokens_bf16(2, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 1, 1, 1, 1, 4, stream()) != 0


# ------------------------------------------------------------------------------------------------ 5. integration
def test_generate_decodes_and_tokenizes_through_a_bf16_tokenizer():
    """The models of test_gpu_decode.test_generate_returns_the_decoded_video with a bf16 tokenizer."""
    kw = dict(dim=32, dim_latent=8, patch_size=4, image_size=16, num_latent_tokens=6, decoder_depth=2, time_block_every=2, attn_heads=2)
    tok = cases.fresh(kw, seed=3, matmul_dtype='bf16')
    torch.manual_seed(0)
    m = randomize_weights(DynamicsWorldModel(dim=64, dim_latent=8, depth=4, time_block_every=2, attn_heads=2, num_discrete_actions=4, video_tokenizer=tok))
    assert m.video_tokenizer.matmul_dtype == 'bf16' and m.matmul_dtype == 'fp32'
    m = m.cuda()
    cfg = oracle_config(m)
    nz = make_noise(cfg, 3, 2, 11)
    nz['video'] = torch.randn(2, 3, 3, 16, 16, generator=torch.Generator().manual_seed(2))
    e = m.generate(3, batch_size=2, return_for_policy_optimization=True, return_terminals=False, noise=nz)
    assert e.video.shape == (2, 3, 3, 16, 16)
    tc = cases.oracle_config(kw)
    W = {k: v.detach().cpu() for k, v in m.video_tokenizer.state_dict().items()}
    lat = e.latents.cpu()
    run = lambda nudge: dict(decode=restate.tokenizer_decode(tc, {k: (v * (1. + nudge) if v.is_floating_point() and not k.endswith('inv_freq') else v) for k, v in W.items()},
                                                             lat * (1. + nudge), nz['video'] * (1. + nudge)))
    with torch.no_grad():
        ref = run(0.)
        E = cases.envelope(run, ref)['decode']
    for metric, f in cases.METRICS.items():
        d, b = f(e.video, ref['decode']), cases.bound(E[metric])
        print(f'generate video {metric}: {d:.3e}  E_max {E[metric]:.3e}  bound {b:.3e}')
        assert d <= b, (metric, d, b)
    assert not torch.allclose(e.video.cpu(), ref['decode'], atol=1e-6, rtol=0.), 'bf16 ran'
    # a video prompt goes through the bf16 encoder
    prompt = torch.rand(2, 3, 2, 16, 16, generator=torch.Generator().manual_seed(4))
    z = m.generate(3, batch_size=2, prompt=prompt, return_decoded_video=False, noise=make_noise(cfg, 3, 2, 12))
    assert z.shape == (2, 3, 6, 8) and torch.isfinite(z).all()


# ------------------------------------------------------------------------------------------------ 6. refusal
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('value', [2, 3])
def test_the_plane_modes_stay_refused(mode, value):
    lib = _lib.load()
    c = cases.build('B')._make_config(mode, (1, 1))
    c.matmul_bf16 = value
    eng = C.c_void_p()
    with pytest.raises(_lib.D4Error, match=f'matmul_bf16={value}'):
        _lib.check(lib.d4_engine_create(C.byref(c), C.byref(eng)))
    c.matmul_bf16 = 1
    _lib.check(lib.d4_engine_create(C.byref(c), C.byref(eng)))
    lib.d4_engine_destroy(eng)
