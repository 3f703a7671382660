"""GPU: bf16 products in the wide-frame inference attention — wide_attn_bf16_kernel<DH> (csrc/attn_wide_bf16.hip) through
d4_small_attn_wide_bf16, and the engine / tokenizer option `attn_products='bf16'` that routes attentions of more than 64 items per
side to it.

Operator: every case of tests/wide_bf16_cases.py against the EXACT float64 reference of tests/attn_core_ref.py within BOUND16 = 2 x E16
(tests/test_wide_bf16_host.py measures E16 on the CPU from an emulation of the kernel's arithmetic contract and asserts that the inputs
see every mutation at 4 x BOUND16), with the buffers, NaN guards and checks of test_gpu_attn_cores.py: the form recorded under the family
"wide_attn_bf16", nothing written outside the output rows, no operand gap read, the bf16 copy bit for bit, two runs the same bits.

Engine: no sampled index may flip, so the comparisons with the oracle run the inference forward (return_pred_only).  The oracle is
evaluated twice on the CPU, as is and with restate.attend wrapped here (oracle/ untouched) so that q, k', v' and the softmax numerators
of an attention with more than 64 items on a side are rounded to bf16; D_emu is the distance of the two relative to max-abs, and the
engine with the option must be within 3 x D_emu + 2e-4 of the plain oracle (the scheme of DESIGN.md 8) and differ from the engine
without it."""
import ctypes as C
import functools

import pytest
import torch

import attn_core_cases as K
import test_gpu_attn_cores as A
import wide_bf16_cases as B
from dreamer4_amd import _lib
from oracle import restate
from test_gpu_wide_infer import TOK, _image, _plain_cases, switch
from util import make_noise, oracle_config, oracle_weights, small_model

pytestmark = pytest.mark.gpu

SEEN = set()
WIDE_FORMS = {'wide_attn_kernel<16>', 'wide_attn_kernel<32>', 'wide_attn_kernel<64>'}
BF16_FORMS = {'wide_attn_bf16_kernel<16>', 'wide_attn_bf16_kernel<32>', 'wide_attn_bf16_kernel<64>'}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


class _Wide16:
    """test_gpu_attn_cores.small_attn_call with d4_small_attn_wide_bf16 in the place of d4_small_attn (one parameter list; the helper
    uses nothing else of its `lib` argument)"""

    def __init__(self, lib):
        self.d4_small_attn = lib.d4_small_attn_wide_bf16


def call16(lib, c, d, **kw):
    return A.small_attn_call(_Wide16(lib), c, d, **kw)


def form16(lib):
    f = lib.d4_debug_last_form(b'wide_attn_bf16')
    assert f is not None, 'no wide_attn_bf16 form recorded'
    SEEN.add(f.decode())
    return f.decode()


def family(lib, name):
    n = lib.d4_debug_forms(name.encode(), 0, None)
    names = set()
    for i in range(n):
        s = C.c_char_p()
        assert lib.d4_debug_forms(name.encode(), i, C.byref(s)) == n
        names.add(s.value.decode())
    return names


# ------------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize('c', B.WIDE16, ids=[c['name'] for c in B.WIDE16])
def test_wide_attn_bf16(lib, c):
    d = K.small_attn_inputs(c)
    rc, out, out_b, geom = call16(lib, c, d)
    _lib.check(rc)
    assert form16(lib) == c['form'] == f"wide_attn_bf16_kernel<{c['dh']}>"
    err = A.check_image(out.dev, _image(c, d, out, geom), B.BOUND16)
    print(f"wide_attn_bf16 {c['name']}: err {err:.3e} (E16 {B.E16:.3e}, bound {B.BOUND16:.3e})")
    if out_b is not None:
        A.check_bf16_copy(out, out_b)
    rc, again, again_b, _ = call16(lib, c, d)
    _lib.check(rc)
    assert torch.equal(A.bits(out.dev), A.bits(again.dev)), 'two runs differ in the output bits'
    if out_b is not None:
        assert torch.equal(A.bits(out_b.dev), A.bits(again_b.dev))


def test_forms_have_a_family_of_their_own(lib):
    assert family(lib, 'wide_attn_bf16') == BF16_FORMS
    assert family(lib, 'wide_attn') == WIDE_FORMS
    assert SEEN == BF16_FORMS, SEEN                                            # (after the operator cases: every head dim ran)


def test_forced_bf16_core_runs_the_small_attn_table(lib):
    """debug switch on: every aligned, unrestricted case of the small_attn table on the bf16 core, within BOUND16"""
    cases = _plain_cases()
    assert len(cases) >= 40 and {c['dh'] for c in cases} == {16, 32, 64} and any(max(c['nq'], c['nk']) <= 16 for c in cases)
    worst = (0., '')
    with switch(lib, 'small_attn_wide', 1):
        for c in cases:
            d = K.small_attn_inputs(c)
            rc, out, out_b, geom = call16(lib, c, d)
            _lib.check(rc)
            assert form16(lib) == f"wide_attn_bf16_kernel<{c['dh']}>", c['name']
            err = A.check_image(out.dev, _image(c, d, out, geom), B.BOUND16)
            worst = max(worst, (err, c['name']))
            if out_b is not None:
                A.check_bf16_copy(out, out_b)
    print(f'forced bf16 core on the small_attn table: worst {worst[0]:.3e} ({worst[1]}), bound {B.BOUND16:.3e}')
    assert lib.d4_debug_switch(b'small_attn_wide', 0) == 0                      # (restored)


def test_bf16_option_changes_nothing_at_64_or_fewer_items(lib):
    """switch off: at <= 64 items per side d4_small_attn_wide_bf16 picks the form d4_small_attn picks and writes the same bits"""
    cases = _plain_cases(small_only=True)
    assert len(cases) >= 30
    for c in cases:
        d = K.small_attn_inputs(c)
        rc, out, out_b, _ = A.small_attn_call(lib, c, d)
        _lib.check(rc)
        form = lib.d4_debug_last_form(b'small_attn').decode()
        assert form == c['form']
        rc, out_w, out_wb, _ = call16(lib, c, d)
        _lib.check(rc)
        assert lib.d4_debug_last_form(b'small_attn').decode() == form, c['name']
        assert torch.equal(A.bits(out.dev), A.bits(out_w.dev)), c['name']
        if out_b is not None:
            assert torch.equal(A.bits(out_b.dev), A.bits(out_wb.dev)), c['name']


def test_wide_attn_bf16_refuses_what_the_wide_core_refuses(lib):
    by = {c['name']: c for c in B.WIDE16}
    c = by['cross-1x1024']                                   # one key more than the cap (the operands hold 1024: nothing is launched)
    rc, out, _, _ = call16(lib, c, K.small_attn_inputs(c), nk_arg=1025)
    A._refused(lib, rc, out, '1024')
    c = by['self-65-dh64']                                   # the core reads its rows as float4
    rc, out, _, _ = call16(lib, c, K.small_attn_inputs(c), q_off=1)
    A._refused(lib, rc, out, '16-byte aligned')
    rc, out, _, _ = call16(lib, c, K.small_attn_inputs(c), restrict=(1, 4, 0))
    A._refused(lib, rc, out, 'query restriction')
    c = dict(by['cross-70x200-ms3'], belief=1)
    rc, out, _, _ = call16(lib, c, K.small_attn_inputs(c))
    A._refused(lib, rc, out, 'belief')
    rc, out, _, _ = call16(lib, by['self-80-dh16'], K.small_attn_inputs(by['self-80-dh16']), dh_arg=48)
    A._refused(lib, rc, out, 'head dim 48')
    c = dict(by['cross-5x200-ms3'], ms=6)                    # more specials than queries: the special block is the tail of both sides
    rc, out, _, _ = call16(lib, c, K.small_attn_inputs(c))
    A._refused(lib, rc, out, '6 special items')


# ------------------------------------------------------------------------------------------------------------------- engine
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    return ((a - b).abs().max() / b.abs().max()).item()


_attend = restate.attend


def attend_bf16(q, k, v, softclamp_value=None, mask=None, causal=False):
    """restate.attend with the roundings of the bf16 core where it runs: a side of more than 64 items (k and v arrive prepared)"""
    if max(q.shape[-2], k.shape[-2]) <= 64:
        return _attend(q, k, v, softclamp_value=softclamp_value, mask=mask, causal=causal)
    assert not causal
    r = lambda t: t.to(torch.bfloat16).to(t.dtype)
    sim = torch.einsum('bhid,bhjd->bhij', r(q), r(k)) * q.shape[-1] ** -0.5
    if softclamp_value is not None:
        sim = restate.softclamp(sim, softclamp_value)
    if mask is not None:
        sim = sim.masked_fill(~mask, -torch.finfo(sim.dtype).max)
    p = torch.exp(sim - sim.amax(-1, keepdim=True))
    return torch.einsum('bhij,bhjd->bhid', r(p), r(v)) / p.sum(-1, keepdim=True)


class emulated:
    def __enter__(self):
        restate.attend = attend_bf16

    def __exit__(self, *exc):
        restate.attend = _attend


def _forward_inputs(m, B_=2, T=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B_, T, m.num_latent_tokens, m.dim_latent, generator=g)
    sig = torch.randint(0, m.max_steps, (B_, T), generator=g)
    acts = torch.randint(0, 4, (B_, T, 1), generator=g)
    return lat, sig, acts


@functools.lru_cache(maxsize=None)
def oracle_pair(name):
    """(pred, agent) of the plain oracle and of the emulating one, and D_emu per tensor, for the forward inputs of configuration `name`"""
    m = small_model(**B.ENGINE[name], wide_frames=True, attn_products='bf16')
    cfg, Wt = oracle_config(m), oracle_weights(m)
    lat, sig, acts = _forward_inputs(m)
    with torch.no_grad():
        plain = restate.wm_forward(cfg, Wt, lat, sig, 4, acts)[:2]
        with emulated():
            emu = restate.wm_forward(cfg, Wt, lat, sig, 4, acts)[:2]
    d = tuple(rel(e, p) for e, p in zip(emu, plain))
    assert all(x > 0. for x in d), 'the emulation changed nothing: no attention of this configuration has a side above 64'
    return plain, d


@pytest.mark.parametrize('name', sorted(B.ENGINE))
def test_bf16_products_forward_vs_oracle(name):
    (pred_o, agent_o), (d_pred, d_agent) = oracle_pair(name)
    outs = {}
    for prod in ('fp32', 'bf16'):
        m = small_model(**B.ENGINE[name], wide_frames=True, attn_products=prod).cuda()
        lat, sig, acts = _forward_inputs(m)
        pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4, discrete_actions=acts)
        outs[prod] = (pred.cpu(), agent.cpu())
    e_pred, e_agent = rel(outs['bf16'][0], pred_o), rel(outs['bf16'][1], agent_o)
    f_pred, f_agent = rel(outs['fp32'][0], pred_o), rel(outs['fp32'][1], agent_o)
    print(f'{name}: pred D_emu {d_pred:.3e} engine {e_pred:.3e} (fp32 products {f_pred:.3e}); agent D_emu {d_agent:.3e} engine {e_agent:.3e} '
          f'(fp32 products {f_agent:.3e})')
    assert e_pred <= 3 * d_pred + 2e-4 and e_agent <= 3 * d_agent + 2e-4
    assert not torch.equal(outs['bf16'][0], outs['fp32'][0]) and not torch.equal(outs['bf16'][1], outs['fp32'][1]), 'the option changed nothing'


def test_bf16_products_generate_runs(lib):
    m = small_model(**B.ENGINE['A'], wide_frames=True, attn_products='bf16').cuda()
    T, Bn = 3, 3
    nz = make_noise(oracle_config(m), T, Bn, 77)
    e = m.generate(T, batch_size=Bn, return_for_policy_optimization=True, noise=nz)
    assert lib.d4_debug_last_form(b'wide_attn_bf16').decode() == 'wide_attn_bf16_kernel<64>'
    assert e.latents.shape == (Bn, T, m.num_latent_tokens, m.dim_latent) and e.agent_embed.shape[:2] == (Bn, T)
    assert e.rewards.shape[0] == Bn and e.values.shape[0] == Bn and e.actions.discrete.shape[:2] == (Bn, T) and e.lens.shape == (Bn,)
    for t in (e.latents, e.agent_embed, e.rewards, e.values, e.log_probs.discrete):
        assert torch.isfinite(t).all()


def test_bf16_products_eager_and_graph_replayed_frames_are_bit_identical(monkeypatch):
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)        # read at engine creation
        m = small_model(**B.ENGINE['B'], wide_frames=True, attn_products='bf16').cuda()
        nz = make_noise(oracle_config(m), 4, 1, 3)
        outs.append(m.generate(4, batch_size=1, return_for_policy_optimization=True, noise=nz))
    a, b = outs
    assert torch.equal(a.latents, b.latents) and torch.equal(a.agent_embed, b.agent_embed) and torch.equal(a.values, b.values)
    assert torch.equal(a.rewards, b.rewards) and torch.equal(a.actions.discrete, b.actions.discrete) and torch.equal(a.log_probs.discrete, b.log_probs.discrete)


def test_bf16_products_forward_parallel_tracks_cached_sequential():
    """the two paths batch their frames differently, and a last-bit difference in a score can flip a bf16 rounding: the bound is this
    configuration's own 3 x D_emu + 2e-4, relative to max-abs"""
    _, (d_pred, d_agent) = oracle_pair('B')
    m = small_model(**B.ENGINE['B'], wide_frames=True, attn_products='bf16').cuda()
    lat, sig, acts = _forward_inputs(m, T=3)
    T = lat.shape[1]
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4, discrete_actions=acts)
    tc, seq, preds = None, [], []
    for i in range(T):
        a = None if i == 0 else acts[:, i - 1:i]
        p, (ag, tc) = m(latents=lat[:, i:i + 1], signal_levels=sig[:, i:i + 1], step_sizes=4, discrete_actions=a, time_cache=tc)
        seq.append(ag); preds.append(p)
    assert agent.abs().max().item() > 1e-2
    e_agent, e_pred = rel(torch.cat(seq, 1), agent), rel(torch.cat(preds, 1), pred)
    print(f'parallel against cached sequential: pred {e_pred:.3e} (bound {3 * d_pred + 2e-4:.3e}), agent {e_agent:.3e} (bound {3 * d_agent + 2e-4:.3e})')
    assert e_pred <= 3 * d_pred + 2e-4 and e_agent <= 3 * d_agent + 2e-4


def test_bf16_products_leave_a_small_model_bit_identical():
    outs = []
    for prod in ('fp32', 'bf16'):
        m = small_model(wide_frames=True, attn_products=prod).cuda()
        nz = make_noise(oracle_config(m), 4, 3, 5)
        outs.append(m.generate(4, batch_size=3, return_for_policy_optimization=True, noise=nz))
    a, b = outs
    assert torch.equal(a.latents, b.latents) and torch.equal(a.agent_embed, b.agent_embed) and torch.equal(a.values, b.values)
    assert torch.equal(a.rewards, b.rewards) and torch.equal(a.actions.discrete, b.actions.discrete) and torch.equal(a.log_probs.discrete, b.log_probs.discrete)


def test_engine_refuses_bf16_products_without_wide_frames(lib):
    """d4_config.wide_frames is a bit set: bit 1 without bit 0 (and anything above 3) is refused at d4_engine_create, before any launch"""
    m = small_model(wide_frames=True, attn_products='bf16')
    for value, frag in ((2, 'need wide frames'), (4, 'wide_frames=4'), (7, 'wide_frames=7')):
        c = m._make_config((1, 4, 1, 0))
        assert c.wide_frames == 3
        c.wide_frames = value
        eng = C.c_void_p()
        assert lib.d4_engine_create(C.byref(c), C.byref(eng)) != 0 and not eng.value
        assert frag in lib.d4_last_error().decode(), lib.d4_last_error().decode()


def test_bf16_engine_with_bf16_products_tracks_fp32():
    """matmul_dtype='bf16' with the option, the rollout of test_gpu_wide_infer.test_wide_bf16_engine_tracks_fp32: that test's bounds (3e-2 on
    the latents, 0.2 on the values) plus 3 x D_emu of each tensor's scale"""
    _, (d_pred, d_agent) = oracle_pair('A')
    a = small_model(**B.ENGINE['A'], wide_frames=True)
    b = small_model(**B.ENGINE['A'], wide_frames=True, matmul_dtype='bf16', attn_products='bf16')
    b.load_state_dict(a.state_dict())
    a, b = a.cuda(), b.cuda()
    nz = make_noise(oracle_config(a), 4, 3, 7)
    kw = dict(return_rewards_per_frame=True, return_agent_actions=True, return_log_probs_and_values=True, noise=nz)
    ea, eb = a.generate(4, batch_size=3, **kw), b.generate(4, batch_size=3, **kw)
    d, dv = (ea.latents - eb.latents).abs().max().item(), (ea.values - eb.values).abs().max().item()
    sl, sv = ea.latents.abs().max().item(), ea.values.abs().max().item()
    print(f'bf16 engine + bf16 products against fp32 at config A: latents {d:.3e} at scale {sl:.3e}, values {dv:.3e} at scale {sv:.3e} '
          f'(D_emu {d_pred:.3e} / {d_agent:.3e})')
    assert 0. < d < 3e-2 + 3 * d_pred * sl, d            # not bit-identical (it really ran in bf16), and close
    assert dv < 0.2 + 3 * d_agent * sv                   # values live on [-20, 20]
    assert all(torch.isfinite(t).all() for t in (eb.latents, eb.values, eb.rewards))


# ------------------------------------------------------------------------------------------------------------------- tokenizer
def _tokenizer(prod):
    from test_gpu_decode import _fresh
    tok = _fresh(dict(TOK, wide_frames=True, attn_products=prod))
    with torch.no_grad():
        tok.latent_tokens.mul_(30.)
    return tok


def test_bf16_products_tokenizer_decode_and_tokenize():
    """192 patches + 70 latents per frame: the option on against off, within 3 x D_emu + 2e-4 of the oracle's own emulation"""
    tok = _tokenizer('fp32')
    tc, Wt = restate.TokenizerConfig(**TOK), {k: v.detach().clone() for k, v in tok.state_dict().items()}
    Bn, T = 2, 2
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(Bn, T, TOK['num_latent_tokens'], TOK['dim_latent'], generator=g).clamp(-1, 1)
    noise = torch.randn(Bn, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    video = torch.rand(Bn, tc.channels, T, tc.image_height, tc.image_width, generator=g)
    with torch.no_grad():
        ref_dec, ref_tok = restate.tokenizer_decode(tc, Wt, lat, noise), restate.tokenizer_tokenize(tc, Wt, video)
        with emulated():
            emu_dec, emu_tok = restate.tokenizer_decode(tc, Wt, lat, noise), restate.tokenizer_tokenize(tc, Wt, video)
    d_dec, d_tok = rel(emu_dec, ref_dec), rel(emu_tok, ref_tok)
    assert d_dec > 0. and d_tok > 0.
    outs = {}
    for prod in ('fp32', 'bf16'):
        t = _tokenizer(prod).cuda()
        outs[prod] = (t.decode(lat, noise=noise).cpu(), t.tokenize(video).cpu())
    e_dec, e_tok = rel(outs['bf16'][0], outs['fp32'][0]), rel(outs['bf16'][1], outs['fp32'][1])
    print(f'tokenizer: decode D_emu {d_dec:.3e} on-off {e_dec:.3e}; tokenize D_emu {d_tok:.3e} on-off {e_tok:.3e}')
    assert 0. < e_dec <= 3 * d_dec + 2e-4 and 0. < e_tok <= 3 * d_tok + 2e-4
    assert rel(outs['bf16'][0], ref_dec) <= 3 * d_dec + 2e-4 and rel(outs['bf16'][1], ref_tok) <= 3 * d_tok + 2e-4
