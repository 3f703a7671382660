"""GPU: wide frames in inference — the tiled matrix-pipe attention core wide_attn_kernel<DH> (csrc/attn_wide_mfma.hip)
through d4_small_attn_wide, and the engine / tokenizer options `wide_frames` that route attentions of more than 64 items per side to it.

Operator: every case of tests/wide_infer_cases.py against the float64 reference of tests/attn_core_ref.py within BOUND['small_attn']
(the host test asserts that bound's E32 holds at these shapes), with the buffers, NaN guards and checks of test_gpu_attn_cores.py: the
form recorded under the family "wide_attn", nothing written outside the output rows, no operand gap read, the bf16 copy bit for bit,
two runs the same bits.  With the debug switch "small_attn_wide" the core also runs the small_attn table's aligned, unrestricted cases;
without it those at <= 64 items per side take the forms of d4_small_attn, bit for bit.

Engine: four models beyond today's 64-token limits against the oracle (restate.generate) under injected noise, every trajectory well
posed; the parallel forward against the cached sequential one; eager against graph-replayed frames; the option on a model that does
not need it; the bf16 engine; the tokenizer's decoder and encoder at 262 tokens per frame."""
import ctypes as C

import pytest
import torch

import attn_core_cases as K
import test_gpu_attn_cores as A
import wide_infer_cases as W
from dreamer4_amd import _lib
from oracle import restate
from util import make_noise, oracle_config, oracle_weights, rollout_parity, small_model

pytestmark = pytest.mark.gpu

SEEN = set()


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


class _Wide:
    """test_gpu_attn_cores.small_attn_call with d4_small_attn_wide in the place of d4_small_attn.  This relies on that helper using
    nothing of its `lib` argument but the attribute `d4_small_attn` (the two entry points have one parameter list): a helper that
    comes to touch another attribute fails here with an AttributeError, not silently"""

    def __init__(self, lib):
        self.d4_small_attn = lib.d4_small_attn_wide


def wide_call(lib, c, d, **kw):
    return A.small_attn_call(_Wide(lib), c, d, **kw)


def wide_form(lib):
    f = lib.d4_debug_last_form(b'wide_attn')
    assert f is not None, 'no wide_attn form recorded'
    SEEN.add(f.decode())
    return f.decode()


def _image(c, d, out, geom):
    G, nq_out, hd, ogs, ois = geom
    want = A.Buf(out.size).host.double()
    want.as_strided((G, nq_out, hd), (ogs, ois, 1), A.GUARD).copy_(K.small_attn_expect(c, d).permute(0, 2, 1, 3).reshape(G, nq_out, hd))
    return want


class switch:
    def __init__(self, lib, name, value):
        self.lib, self.name, self.value = lib, name.encode(), value

    def __enter__(self):
        self.old = self.lib.d4_debug_switch(self.name, self.value)
        assert self.old >= 0, 'unknown debug switch'

    def __exit__(self, *exc):
        self.lib.d4_debug_switch(self.name, self.old)


# ------------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize('c', W.WIDE, ids=[c['name'] for c in W.WIDE])
def test_wide_attn(lib, c):
    d = K.small_attn_inputs(c)
    rc, out, out_b, geom = wide_call(lib, c, d)
    _lib.check(rc)
    assert wide_form(lib) == c['form']
    err = A.check_image(out.dev, _image(c, d, out, geom), W.BOUND)
    print(f"wide_attn {c['name']}: err {err:.3e} (bound {W.BOUND:.3e})")
    if out_b is not None:
        A.check_bf16_copy(out, out_b)
    rc, again, again_b, _ = wide_call(lib, c, d)
    _lib.check(rc)
    assert torch.equal(A.bits(out.dev), A.bits(again.dev)), 'two runs differ in the output bits'
    if out_b is not None:
        assert torch.equal(A.bits(out_b.dev), A.bits(again_b.dev))


def _plain_cases(small_only=False):
    return [c for c in K.SMALL_ATTN if c['align'] == 'ok' and c['restrict'] is None and (not small_only or max(c['nq'], c['nk']) <= 64)]


def test_forced_wide_core_runs_the_small_attn_table(lib):
    """debug switch on: every aligned, unrestricted case of the small_attn table on the wide core, within the same bound"""
    cases = _plain_cases()
    assert len(cases) >= 40 and {c['dh'] for c in cases} == {16, 32, 64} and any(max(c['nq'], c['nk']) <= 16 for c in cases)
    with switch(lib, 'small_attn_wide', 1):
        for c in cases:
            d = K.small_attn_inputs(c)
            rc, out, out_b, geom = wide_call(lib, c, d)
            _lib.check(rc)
            assert wide_form(lib) == f"wide_attn_kernel<{c['dh']}>", c['name']
            err = A.check_image(out.dev, _image(c, d, out, geom), W.BOUND)
            print(f"forced {c['name']}: err {err:.3e}")
            if out_b is not None:
                A.check_bf16_copy(out, out_b)
    assert lib.d4_debug_switch(b'small_attn_wide', 0) == 0                      # (restored)


def test_wide_option_changes_nothing_at_64_or_fewer_items(lib):
    """switch off: at <= 64 items per side d4_small_attn_wide picks the form d4_small_attn picks and writes the same bits"""
    cases = _plain_cases(small_only=True)
    assert len(cases) >= 30
    for c in cases:
        d = K.small_attn_inputs(c)
        rc, out, out_b, _ = A.small_attn_call(lib, c, d)
        _lib.check(rc)
        form = lib.d4_debug_last_form(b'small_attn').decode()
        assert form == c['form']
        rc, out_w, out_wb, _ = wide_call(lib, c, d)
        _lib.check(rc)
        assert lib.d4_debug_last_form(b'small_attn').decode() == form, c['name']
        assert torch.equal(A.bits(out.dev), A.bits(out_w.dev)), c['name']
        if out_b is not None:
            assert torch.equal(A.bits(out_b.dev), A.bits(out_wb.dev)), c['name']


def test_wide_attn_refuses_what_it_does_not_implement(lib):
    by = {c['name']: c for c in W.WIDE}
    c = by['cross-1x1024']                                   # one key more than the cap (the operands hold 1024: nothing is launched)
    rc, out, _, _ = wide_call(lib, c, K.small_attn_inputs(c), nk_arg=1025)
    A._refused(lib, rc, out, '1024')
    c = by['self-65-dh64']                                   # the core reads its rows as float4
    rc, out, _, _ = wide_call(lib, c, K.small_attn_inputs(c), q_off=1)
    A._refused(lib, rc, out, '16-byte aligned')
    rc, out, _, _ = wide_call(lib, c, K.small_attn_inputs(c), restrict=(1, 4, 0))
    A._refused(lib, rc, out, 'query restriction')
    c = dict(by['cross-70x200-ms3'], belief=1)
    rc, out, _, _ = wide_call(lib, c, K.small_attn_inputs(c))
    A._refused(lib, rc, out, 'belief')
    rc, out, _, _ = wide_call(lib, by['self-80-dh16'], K.small_attn_inputs(by['self-80-dh16']), dh_arg=48)
    A._refused(lib, rc, out, 'head dim 48')
    c = dict(by['cross-5x200-ms3'], ms=6)                    # more specials than queries: the special block is the tail of both sides
    rc, out, _, _ = wide_call(lib, c, K.small_attn_inputs(c))
    A._refused(lib, rc, out, '6 special items')
    # without the option the launcher keeps its limit and its message
    c = next(c for c in K.SMALL_ATTN if c['name'] == 'wide-self-160')
    rc, out, _, _ = A.small_attn_call(lib, c, K.small_attn_inputs(c), nk_arg=161)
    A._refused(lib, rc, out, '161 keys (max 160)')


def test_every_wide_form_ran(lib):
    n = lib.d4_debug_forms(b'wide_attn', 0, None)
    names = set()
    for i in range(n):
        s = C.c_char_p()
        assert lib.d4_debug_forms(b'wide_attn', i, C.byref(s)) == n
        names.add(s.value.decode())
    assert names == {'wide_attn_kernel<16>', 'wide_attn_kernel<32>', 'wide_attn_kernel<64>'} and SEEN == names, (names, SEEN)


# ------------------------------------------------------------------------------------------------------------------- engine
def close(a, b, atol=2e-4, rtol=1e-4):                       # (the tolerances of test_gpu_generate.py)
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, atol=atol, rtol=rtol), f'max abs diff {(a - b).abs().max().item():.3e}'


@pytest.mark.parametrize('name', sorted(W.ENGINE))
def test_wide_generate_vs_oracle(name):
    m = small_model(**W.ENGINE[name], wide_frames=True)
    cfg, Wt = oracle_config(m), oracle_weights(m)
    B, T = 3, 3
    nz = make_noise(cfg, T, B, 77)
    ref = restate.generate(cfg, Wt, T, batch_size=B, noise=nz)
    e = m.cuda().generate(T, batch_size=B, return_for_policy_optimization=True, noise=nz)
    rp = rollout_parity(e, ref, nz, cfg)
    print(name, rp)
    assert rp['well_posed_trajectories'] == 3 and ref['latents'].shape[1] == T and e.latents.shape[1] == T
    assert torch.equal(e.actions.discrete.cpu(), ref['actions']) and torch.equal(e.lens.cpu(), ref['lens'])
    close(e.latents, ref['latents']); close(e.agent_embed, ref['agent_embed']); close(e.rewards, ref['rewards'])
    close(e.values, ref['values']); close(e.log_probs.discrete, ref['log_probs'])


def test_wide_forward_parallel_equals_cached_sequential():
    m = small_model(**W.ENGINE['B'], wide_frames=True).cuda()
    B, T = 2, 3
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(B, T, m.num_latent_tokens, m.dim_latent, generator=g)
    sig = torch.randint(0, m.max_steps, (B, T), generator=g)
    acts = torch.randint(0, 4, (B, T, 1), generator=g)
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4, discrete_actions=acts)
    tc, seq, preds = None, [], []
    for i in range(T):
        a = None if i == 0 else acts[:, i - 1:i]
        p, (ag, tc) = m(latents=lat[:, i:i + 1], signal_levels=sig[:, i:i + 1], step_sizes=4, discrete_actions=a, time_cache=tc)
        seq.append(ag); preds.append(p)
    assert agent.abs().max().item() > 1e-2
    close(torch.cat(seq, 1), agent, atol=1e-5)
    close(torch.cat(preds, 1), pred, atol=1e-5)


def test_wide_eager_and_graph_replayed_frames_are_bit_identical(monkeypatch):
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)        # read at engine creation
        m = small_model(**W.ENGINE['B'], wide_frames=True).cuda()
        nz = make_noise(oracle_config(m), 4, 1, 3)
        outs.append(m.generate(4, batch_size=1, return_for_policy_optimization=True, noise=nz))
    a, b = outs
    assert torch.equal(a.latents, b.latents) and torch.equal(a.agent_embed, b.agent_embed) and torch.equal(a.values, b.values)
    assert torch.equal(a.rewards, b.rewards) and torch.equal(a.actions.discrete, b.actions.discrete) and torch.equal(a.log_probs.discrete, b.log_probs.discrete)


def test_wide_option_leaves_a_small_model_bit_identical():
    outs = []
    for wide in (False, True):
        m = small_model(wide_frames=wide).cuda()
        nz = make_noise(oracle_config(m), 4, 3, 5)
        outs.append(m.generate(4, batch_size=3, return_for_policy_optimization=True, noise=nz))
    a, b = outs
    assert torch.equal(a.latents, b.latents) and torch.equal(a.agent_embed, b.agent_embed) and torch.equal(a.values, b.values)
    assert torch.equal(a.rewards, b.rewards) and torch.equal(a.actions.discrete, b.actions.discrete) and torch.equal(a.log_probs.discrete, b.log_probs.discrete)


def test_wide_model_without_the_option_is_still_refused():
    m = small_model(**W.ENGINE['A']).cuda()
    with pytest.raises(_lib.D4Error, match='at most 64'):
        m.generate(2, batch_size=1)


def test_wide_bf16_engine_tracks_fp32():
    a = small_model(**W.ENGINE['A'], wide_frames=True)
    b = small_model(**W.ENGINE['A'], wide_frames=True, matmul_dtype='bf16')
    b.load_state_dict(a.state_dict())
    a, b = a.cuda(), b.cuda()
    nz = make_noise(oracle_config(a), 4, 3, 7)
    kw = dict(return_rewards_per_frame=True, return_agent_actions=True, return_log_probs_and_values=True, noise=nz)
    ea, eb = a.generate(4, batch_size=3, **kw), b.generate(4, batch_size=3, **kw)
    d = (ea.latents - eb.latents).abs().max().item()
    print(f'bf16 against fp32 at config A: latents {d:.3e}, values {(ea.values - eb.values).abs().max().item():.3e}')
    assert 0. < d < 3e-2, d            # not bit-identical (it really ran in bf16), and close
    assert (ea.values - eb.values).abs().max().item() < 0.2           # values live on [-20, 20]


# ------------------------------------------------------------------------------------------------------------------- tokenizer
TOK = dict(dim=64, dim_latent=8, patch_size=4, image_height=64, image_width=48, num_latent_tokens=70, encoder_depth=2, decoder_depth=2, time_block_every=2,
           attn_heads=2)                                     # 192 patches + 70 latents per frame


def _tokenizer(wide):
    from test_gpu_decode import _fresh
    tok = _fresh(dict(TOK, wide_frames=wide))
    with torch.no_grad():
        tok.latent_tokens.mul_(30.)
    return tok, restate.TokenizerConfig(**TOK), {k: v.detach().clone() for k, v in tok.state_dict().items()}


def test_wide_tokenizer_decode_and_tokenize_vs_oracle():
    from test_gpu_decode import close as close_tok
    tok, tc, Wt = _tokenizer(True)
    B, T = 2, 2
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, T, TOK['num_latent_tokens'], TOK['dim_latent'], generator=g).clamp(-1, 1)
    noise = torch.randn(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    video = torch.rand(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    ref_dec, ref_tok = restate.tokenizer_decode(tc, Wt, lat, noise), restate.tokenizer_tokenize(tc, Wt, video)
    tok = tok.cuda()
    close_tok(tok.decode(lat, noise=noise), ref_dec)
    out = tok.tokenize(video)
    assert out.abs().max().item() < 1. and ref_tok.std().item() > 0.05
    close_tok(out, ref_tok)


def test_wide_tokenizer_without_the_option_is_still_refused():
    tok, tc, _ = _tokenizer(False)
    tok = tok.cuda()
    with pytest.raises(_lib.D4Error, match='at most 64 latent / spatial tokens'):
        tok.decode(torch.zeros(1, 1, TOK['num_latent_tokens'], TOK['dim_latent']))
    with pytest.raises(_lib.D4Error, match='at most 64 latent / spatial tokens'):
        tok.tokenize(torch.zeros(1, tc.channels, 1, tc.image_height, tc.image_width))
