"""GPU: deep trunks in inference — the chunked AttentionPool mix (csrc/pool_mix_deep.hip) through d4_pool_mix_deep, and the
engine / tokenizer option `wide_frames` that routes pools of more than 64 hiddens (depth >= 32) to it.

Operator: every case of tests/deep_pool_cases.py against the float64 reference of tests/attn_core_ref.py within that table's own bound
(8 x its E32; tests/test_deep_pool_host.py asserts the E32 and that the bound sees every mutation), with the checks of
test_gpu_attn_cores.py: the form recorded under the family "pool_mix_deep", the bf16 copy bit for bit, two runs the same bits.  Here EVERY
operand sits between NaN guards in a NaN-filled buffer that holds one more (NaN) hidden and key slab than L, with NaN in the gaps of padded
key / query rows: a hidden or key past L, or a row gap, that is read poisons the output, and nothing but the output rows is written.
The launcher also runs the whole pool_mix table (L <= 64) within that table's bound.

Engine: four models of depth 32 .. 65 against the oracle (restate.generate) under injected noise, every trajectory well posed; the
parallel forward against the cached sequential one; eager against graph-replayed frames; the debug switch that sends the small pools to
the chunked kernel too; the refusals; the bf16 engine with its wide key projection on and off; the fused tail behind the chunked mix; the
tokenizer's decoder and encoder at depth 33; a deep trunk trained one step and then run."""
import ctypes as C

import pytest
import torch

import attn_core_cases as K
import deep_pool_cases as P
import test_gpu_attn_cores as A
from dreamer4_amd import _lib
from oracle import restate
from test_gpu_attn_cores import Buf, bits, stream
from util import make_noise, oracle_config, oracle_weights, rollout_parity, small_model

pytestmark = pytest.mark.gpu

DEV = A.DEV
SEEN = set()
WORST = [0., '']


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def deep_form(lib):
    f = lib.d4_debug_last_form(b'pool_mix_deep')
    assert f is not None, 'no pool_mix_deep form recorded'
    SEEN.add(f.decode())
    return f.decode()


class switch:
    def __init__(self, lib, name, value):
        self.lib, self.name, self.value = lib, name.encode(), value

    def __enter__(self):
        self.old = self.lib.d4_debug_switch(self.name, self.value)
        assert self.old >= 0, 'unknown debug switch'

    def __exit__(self, *exc):
        self.lib.d4_debug_switch(self.name, self.old)


# ------------------------------------------------------------------------------------------------------------------- operator
class DeepRun:
    """The device buffers of one case: every operand a Buf (NaN guards, NaN gaps, one NaN slab past L), uploaded once; call() makes fresh outputs."""

    def __init__(self, c, d):
        M, L, D = c['M'], c['L'], c['D']
        self.c = c
        self.ldk = 256 if not c['kb'] else (512, 256, 776)[c['seed'] % 3]      # bf16 keys: any leading dimension (the engine's wide key image)
        self.ldq = self.ldk if c['qb'] else 264
        k16, q16, h16 = (torch.bfloat16 if f else torch.float32 for f in (c['kb'], c['qb'], c['hb']))
        self.k = Buf((L + 1) * M * self.ldk, dtype=k16)
        self.k.view((L, M, 256), (M * self.ldk, self.ldk, 1)).copy_(d['k'])
        self.q = Buf(M * self.ldq, dtype=q16)
        self.q.view((M, 256), (self.ldq, 1)).copy_(d['q'])
        self.hid = Buf((L + 1) * M * D)
        self.hid.view((L, M, D), (M * D, D, 1)).copy_(d['hid'])
        self.hid_b = None
        if c['hb']:
            self.hid_b = Buf((L + 1) * M * D, dtype=h16)
            self.hid_b.view((L, M, D), (M * D, D, 1)).copy_(d['hid'])
        self.x = None
        if not c['x_last']:
            self.x = Buf(M * (D + 4))
            self.x.view((M, D), (D + 4, 1)).copy_(d['x'])
        self.gw, self.gamma = Buf(4 * D), Buf(4 * 64)
        self.gw.view((4, D), (D, 1)).copy_(d['gate_w'])
        self.gamma.view((4, 64), (64, 1)).copy_(d['gamma'])
        self.operands = [b.upload() for b in (self.k, self.q, self.hid, self.hid_b, self.x, self.gw, self.gamma) if b is not None]
        self.before = [b.dev.clone() for b in self.operands]

    def call(self, lib, *, L=None, D=None, heads=4, no_u=False, entry='d4_pool_mix_deep'):
        c = self.c
        M, Lc, Dc = c['M'], c['L'], c['D']
        xp, ldx = (C.c_void_p(self.hid.ptr.value + 4 * (Lc - 1) * M * Dc), Dc) if c['x_last'] else (self.x.ptr, Dc + 4)
        u = Buf(M * 4 * Dc).upload()
        ub = Buf(M * 4 * Dc, dtype=torch.bfloat16).upload() if c['ub'] else None
        rc = getattr(lib, entry)(None if c['qb'] else self.q.ptr, self.ldq, xp, ldx, self.gw.ptr, None if c['kb'] else self.k.ptr, self.ldk, self.hid.ptr, D or Dc,
                                 self.gamma.ptr, None if no_u else u.ptr, M, L or Lc if L != 0 else 0, heads, c['eps'], None if ub is None else ub.ptr,
                                 self.k.ptr if c['kb'] else None, self.q.ptr if c['qb'] else None, None if self.hid_b is None else self.hid_b.ptr, stream())
        torch.cuda.synchronize()
        return rc, u, ub

    def operands_untouched(self):
        return all(torch.equal(bits(b.dev), bits(o)) for b, o in zip(self.operands, self.before))


@pytest.mark.parametrize('c', P.DEEP, ids=[c['name'] for c in P.DEEP])
def test_pool_mix_deep(lib, c):
    d = K.pool_inputs(c)
    ref = P.deep_expect(c, d)                                                             # [M, 4, D]
    r = DeepRun(c, d)
    rc, u, ub = r.call(lib)
    _lib.check(rc)
    assert deep_form(lib) == c['form']
    want = Buf(u.size).host.double()
    want[A.GUARD:A.GUARD + u.size] = ref.reshape(-1)
    err = A.check_image(u.dev, want, P.BOUND)
    print(f"pool_mix_deep {c['name']}: err {err:.3e} (bound {P.BOUND:.3e})")
    if err > WORST[0]:
        WORST[:] = [err, c['name']]
    if ub is not None:
        A.check_bf16_copy(u, ub)
    rc, again, again_b = r.call(lib)
    _lib.check(rc)
    assert torch.equal(bits(u.dev), bits(again.dev)), 'two runs differ in the output bits'
    if ub is not None:
        assert torch.equal(bits(ub.dev), bits(again_b.dev))
        rc, none, only_b = r.call(lib, no_u=True)                                         # u may be null when u_b is set
        _lib.check(rc)
        assert none.dev.isnan().all() and torch.equal(bits(ub.dev), bits(only_b.dev))
    assert r.operands_untouched(), 'an operand buffer was written'


class _Deep:
    """test_gpu_attn_cores.pool_call with d4_pool_mix_deep in the place of d4_pool_mix (one parameter list): the helper uses nothing of
    its `lib` argument but the attribute `d4_pool_mix`; one that comes to touch another fails here with an AttributeError"""

    def __init__(self, lib):
        self.d4_pool_mix = lib.d4_pool_mix_deep


def test_deep_launcher_runs_the_pool_mix_table(lib):
    """every case of the pool_mix table (L <= 64: a single, ragged chunk) on the chunked launcher, within THAT table's bound"""
    assert len(K.POOL_MIX) >= 60 and max(c['L'] for c in K.POOL_MIX) == 64
    for c in K.POOL_MIX:
        d = K.pool_inputs(c)
        rc, u, ub = A.pool_call(_Deep(lib), c, d)
        _lib.check(rc)
        assert deep_form(lib) == c['form'].replace('pool_mix_', 'pool_mix_deep_'), c['name']
        want = Buf(u.size).host.double()
        want[A.GUARD:A.GUARD + u.size] = K.pool_expect(c, d).reshape(-1)
        err = A.check_image(u.dev, want, K.BOUND['pool_mix'])
        print(f"deep launcher, {c['name']}: err {err:.3e} (bound {K.BOUND['pool_mix']:.3e})")
        if ub is not None:
            A.check_bf16_copy(u, ub)


def test_pool_mix_deep_refuses_what_it_does_not_cover(lib):
    by = {c['name']: c for c in P.DEEP}
    c = by['deep-D1024-L1024-M1-f32']                        # (the operands hold 1024 hiddens + one NaN slab: nothing is launched)
    r = DeepRun(c, K.pool_inputs(c))
    for kw, frag in ((dict(L=1025), 'L=1025'), (dict(L=0), 'L=0'), (dict(D=1028), 'D=1028'), (dict(heads=3), 'heads=3')):
        rc, u, _ = r.call(lib, **kw)
        A._refused(lib, rc, u, frag)
    # d4_pool_mix keeps its limit and its message
    c = by['deep-D64-L65-M1-f32']
    rc, u, _ = DeepRun(c, K.pool_inputs(c)).call(lib, entry='d4_pool_mix')
    A._refused(lib, rc, u, 'L=65')


def test_every_deep_form_ran(lib):
    print(f'worst pool_mix_deep: {WORST[0]:.3e} of bound {P.BOUND:.3e} ({WORST[1]})')
    n = lib.d4_debug_forms(b'pool_mix_deep', 0, None)
    names = set()
    for i in range(n):
        s = C.c_char_p()
        assert lib.d4_debug_forms(b'pool_mix_deep', i, C.byref(s)) == n
        names.add(s.value.decode())
    assert names == P.FORMS and SEEN == names, (sorted(names - SEEN), sorted(SEEN - names))
    # the pool_mix family's list is what it was
    m = lib.d4_debug_forms(b'pool_mix', 0, None)
    assert m == 10 and {c['form'] for c in K.POOL_MIX} == {_form(lib, b'pool_mix', i) for i in range(m)}


def _form(lib, fam, i):
    s = C.c_char_p()
    lib.d4_debug_forms(fam, i, C.byref(s))
    return s.value.decode()


# ------------------------------------------------------------------------------------------------------------------- frame tail
def test_chunked_mix_then_fused_tail_equals_the_separate_gemms(lib):
    """What pool_block runs for a pool of more than 64 hiddens where the per-frame tail applies (dim 512, 192 frames x 15 tokens): pool_mix_deep,
    then d4_frame_pool_tail — against pool_mix_deep followed by the per-head value GEMM (d4_gemm_batched) and the output projection with the
    residual (d4_gemm), which is what it runs elsewhere."""
    import fused_ref as F
    frames, S, D, L = 192, 15, 512, 65
    M = frames * S
    g = torch.Generator().manual_seed(12500)
    n = lambda *s, scale=1.: (torch.randn(*s, generator=g) * scale).to(DEV)
    q, k, hid, gw, gamma = n(M, 256), n(L, M, 256), n(L, M, D), n(4, D, scale=2 * D ** -0.5), n(4, 64, scale=0.2)
    Wv, Wo, resid = n(256, D, scale=D ** -0.5), n(D, 256, scale=1 / 16), n(M, D)
    u = torch.full((M, 4, D), float('nan'), device=DEV)
    xp = C.c_void_p(hid.data_ptr() + 4 * (L - 1) * M * D)
    _lib.check(lib.d4_pool_mix_deep(_lib.ptr(q), 256, xp, D, _lib.ptr(gw), _lib.ptr(k), 256, _lib.ptr(hid), D, _lib.ptr(gamma), _lib.ptr(u), M, L, 4, 1.1920929e-07,
                                    None, None, None, None, stream()))
    assert deep_form(lib) == 'pool_mix_deep_kernel<2>'
    wv_t, wo_t = F.tile16_ref(Wv.cpu(), 256, D).reshape(-1).to(DEV), F.tile16_ref(Wo.cpu(), D, 256).reshape(-1).to(DEV)
    out_t = torch.full((M, D), float('nan'), device=DEV)
    _lib.check(lib.d4_frame_pool_tail(_lib.ptr(u), _lib.ptr(wv_t), _lib.ptr(wo_t), frames, S, D, 4, _lib.ptr(resid), D, _lib.ptr(out_t), D, None, D, 0, 0, 0, stream()))
    att = torch.full((M, 256), float('nan'), device=DEV)
    _lib.check(lib.d4_gemm_batched(_lib.ptr(u), 4 * D, _lib.ptr(Wv), D, _lib.ptr(att), 256, None, None, 0, M, 64, D, 0, 1.1920929e-07, 4, D, 64 * D, 64, stream()))
    out_g = torch.full((M, D), float('nan'), device=DEV)
    _lib.check(lib.d4_gemm(_lib.ptr(att), 256, _lib.ptr(Wo), 256, _lib.ptr(out_g), D, None, _lib.ptr(resid), D, M, D, 256, 0, 1.1920929e-07, stream()))
    torch.cuda.synchronize()
    assert not out_t.isnan().any() and not out_g.isnan().any()
    diff = (out_t - out_g).abs().max().item()
    print(f'mix + fused tail against mix + separate GEMMs: max |diff| {diff:.3e} at scale {out_g.abs().max().item():.3g}')
    assert torch.equal(bits(out_t), bits(out_g)), f'max |diff| {diff:.3e}'


# ------------------------------------------------------------------------------------------------------------------- engine
def close(a, b, atol=2e-4, rtol=1e-4):                       # (the tolerances of test_gpu_generate.py)
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, atol=atol, rtol=rtol), f'max abs diff {(a - b).abs().max().item():.3e}'


@pytest.mark.parametrize('name', sorted(P.ENGINE))
def test_deep_generate_vs_oracle(lib, name):
    m = small_model(**P.ENGINE[name], wide_frames=True)
    cfg, Wt = oracle_config(m), oracle_weights(m)
    B, T = 3, 3
    nz = make_noise(cfg, T, B, 77)
    ref = restate.generate(cfg, Wt, T, batch_size=B, noise=nz)
    e = m.cuda().generate(T, batch_size=B, return_for_policy_optimization=True, noise=nz)
    assert lib.d4_debug_last_form(b'pool_mix_deep') is not None, 'no pool took the chunked kernel'
    rp = rollout_parity(e, ref, nz, cfg)
    print(name, rp)
    assert rp['well_posed_trajectories'] == 3 and ref['latents'].shape[1] == T and e.latents.shape[1] == T
    assert torch.equal(e.actions.discrete.cpu(), ref['actions']) and torch.equal(e.lens.cpu(), ref['lens'])
    close(e.latents, ref['latents']); close(e.agent_embed, ref['agent_embed']); close(e.rewards, ref['rewards'])
    close(e.values, ref['values']); close(e.log_probs.discrete, ref['log_probs'])


def test_deep_forward_parallel_equals_cached_sequential():
    m = small_model(**P.ENGINE['B'], wide_frames=True).cuda()
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


def _same(a, b):
    return (torch.equal(a.latents, b.latents) and torch.equal(a.agent_embed, b.agent_embed) and torch.equal(a.values, b.values) and torch.equal(a.rewards, b.rewards)
            and torch.equal(a.actions.discrete, b.actions.discrete) and torch.equal(a.log_probs.discrete, b.log_probs.discrete))


def test_deep_eager_and_graph_replayed_frames_are_bit_identical(monkeypatch):
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)        # read at engine creation
        m = small_model(**P.ENGINE['B'], wide_frames=True).cuda()
        nz = make_noise(oracle_config(m), 4, 1, 3)
        outs.append(m.generate(4, batch_size=1, return_for_policy_optimization=True, noise=nz))
    assert _same(*outs)


def test_debug_switch_sends_the_small_pools_to_the_chunked_kernel(lib):
    """another summation order, same values: depth 4 (pools of 3 .. 9 hiddens) with every pool on pool_mix_deep against its normal rollout;
    and without the switch the option alone changes no bit"""
    outs = {}
    for key, wide, sw in (('plain', False, 0), ('option', True, 0), ('forced', True, 1)):
        with switch(lib, 'pool_mix_deep', sw):
            m = small_model(wide_frames=wide).cuda()
            nz = make_noise(oracle_config(m), 4, 3, 5)
            outs[key] = m.generate(4, batch_size=3, return_for_policy_optimization=True, noise=nz)
            if sw:
                assert lib.d4_debug_last_form(b'pool_mix_deep') is not None
    assert lib.d4_debug_switch(b'pool_mix_deep', 0) == 0                        # (restored)
    assert _same(outs['plain'], outs['option'])
    a, b = outs['forced'], outs['plain']
    assert torch.equal(a.actions.discrete, b.actions.discrete)
    for f in ('latents', 'agent_embed', 'values', 'rewards'):
        close(getattr(a, f), getattr(b, f), atol=2e-4)
    close(a.log_probs.discrete, b.log_probs.discrete, atol=2e-4)
    assert not torch.equal(a.agent_embed, b.agent_embed), 'the switch changed nothing: the chunked kernel did not run'


def test_deep_model_without_the_option_is_still_refused():
    m = small_model(**P.ENGINE['A']).cuda()
    with pytest.raises(_lib.D4Error, match='exceed 64'):
        m.generate(2, batch_size=1)


def test_engine_create_names_the_cap_and_the_mix_path_condition(lib):
    m = small_model(wide_frames=True)

    def refused(**over):
        c = m._make_config((1, 4, 1, 0))
        for k, v in over.items():
            setattr(c, k, v)
        eng = C.c_void_p()
        rc = lib.d4_engine_create(C.byref(c), C.byref(eng))
        assert rc != 0 and not eng.value
        return lib.d4_last_error().decode()

    assert '1024' in refused(depth=512) and '1025 pooled hiddens' in refused(depth=512)
    msg = refused(depth=32, dim=1028)
    assert 'pool_heads == 4 && dim <= 1024' in msg and 'dim=1028' in msg, msg
    assert 'pool_heads == 4 && dim <= 1024' in refused(depth=32, pool_heads=2)
    assert 'exceed 64' in refused(depth=32, wide_frames=0)
    c = m._make_config((1, 4, 1, 0))                         # depth 511 = 1023 hiddens is accepted (creation allocates nothing on the device)
    c.depth = 511
    eng = C.c_void_p()
    _lib.check(lib.d4_engine_create(C.byref(c), C.byref(eng)))
    lib.d4_engine_destroy(eng)


@pytest.mark.parametrize('wide_keys', (1, 0))
def test_deep_bf16_engine_tracks_fp32(lib, wide_keys):
    a = small_model(**P.ENGINE['A'], wide_frames=True)
    b = small_model(**P.ENGINE['A'], wide_frames=True, matmul_dtype='bf16')
    b.load_state_dict(a.state_dict())
    a, b = a.cuda(), b.cuda()
    nz = make_noise(oracle_config(a), 4, 3, 7)
    kw = dict(return_rewards_per_frame=True, return_agent_actions=True, return_log_probs_and_values=True, noise=nz)
    ea = a.generate(4, batch_size=3, **kw)
    with switch(lib, 'pool_wide_keys', wide_keys):
        eb = b.generate(4, batch_size=3, **kw)
        assert lib.d4_debug_last_form(b'pool_mix_deep').decode().endswith(',bf16>')
    d = (ea.latents - eb.latents).abs().max().item()
    print(f'bf16 (pool_wide_keys {wide_keys}) against fp32 at config A: latents {d:.3e}, values {(ea.values - eb.values).abs().max().item():.3e}')
    assert 0. < d < 3e-2, d            # not bit-identical (it really ran in bf16), and close
    assert (ea.values - eb.values).abs().max().item() < 0.2           # values live on [-20, 20]


def test_deep_trunk_trained_one_step_then_run():
    """configuration B with train_wide_frames=True and wide_frames=True: the training forward + backward (the tiled cross-attention core over up
    to 67 hiddens), then the same module generates on the engine"""
    from math import log2
    m = small_model(**P.ENGINE['B'], train_wide_frames=True, wide_frames=True).cuda()
    B, T = 1, 2
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(B, T, *m.latent_shape, generator=g)
    actions = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in tuple(m.num_discrete_actions)], dim=-1)
    step_log2 = torch.randint(1, int(log2(m.max_steps)), (B,), generator=g)
    nss = (2 ** step_log2)[:, None]
    sig = torch.randint(0, m.max_steps, (B, T), generator=g) // nss * nss
    draws = dict(shortcut_train=True, step_sizes_log2=step_log2, signal_levels=sig, noise=torch.randn(lat.shape, generator=g))
    total, _ = m(latents=lat, discrete_actions=actions, return_all_losses=True, draws=draws, add_autoregressive_action_loss=False)
    assert torch.isfinite(total).all()
    total.backward()
    trunk = {k: p for k, p in m.named_parameters() if k.startswith('transformer.')}
    pools = [k for k in trunk if '.attn_pools.' in k or '.final_attn_pool.' in k]
    assert len(trunk) >= 20 * m.depth and len(pools) >= 5 * m.depth
    unreached = 'transformer.final_special_cross_attn.fn.to_learned_value_residual_mix.'       # (that attention takes no value residual)
    bad = [k for k, p in trunk.items() if not k.startswith(unreached) and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad[:5]
    assert all(trunk[k].grad.abs().max().item() > 0 for k in pools if k.endswith('to_q.weight') or k.endswith('to_out.weight'))
    m.zero_grad(set_to_none=True)
    e = m.generate(2, batch_size=1, return_for_policy_optimization=True, noise=make_noise(oracle_config(m), 2, 1, 9))
    assert e.latents.shape[1] == 2 and torch.isfinite(e.latents).all() and torch.isfinite(e.agent_embed).all()


# ------------------------------------------------------------------------------------------------------------------- tokenizer
TOK = dict(dim=64, dim_latent=8, patch_size=4, image_height=16, image_width=12, num_latent_tokens=6, encoder_depth=33, decoder_depth=33, time_block_every=3,
           attn_heads=2)                                     # 12 patches + 6 latents per frame; pools over up to 67 hiddens


def test_deep_tokenizer_decode_and_tokenize_vs_oracle():
    from test_gpu_decode import _fresh, close as close_tok
    tok = _fresh(dict(TOK, wide_frames=True))
    with torch.no_grad():
        tok.latent_tokens.mul_(30.)
    tc, Wt = restate.TokenizerConfig(**TOK), {k: v.detach().clone() for k, v in tok.state_dict().items()}
    B, T = 2, 2
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, T, TOK['num_latent_tokens'], TOK['dim_latent'], generator=g).clamp(-1, 1)
    noise = torch.randn(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    video = torch.rand(B, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    ref_dec, ref_tok = restate.tokenizer_decode(tc, Wt, lat, noise), restate.tokenizer_tokenize(tc, Wt, video)
    tok = tok.cuda()
    close_tok(tok.decode(lat, noise=noise), ref_dec)
    out = tok.tokenize(video)
    assert ref_tok.std().item() > 0.01
    close_tok(out, ref_tok)


def test_deep_tokenizer_without_the_option_is_still_refused():
    from test_gpu_decode import _fresh
    tok = _fresh(dict(TOK)).cuda()
    with pytest.raises(_lib.D4Error, match='exceed 64'):
        tok.decode(torch.zeros(1, 1, TOK['num_latent_tokens'], TOK['dim_latent']))
