"""GPU: the bf16-product form of the tiled attention core of the training path (csrc/attn_tiled_bf16.hip), opt-in through
d4_train_attn_products_set / `attn_products='bf16'` / `DynamicsWorldModel(train_attn_products='bf16')`.

Operator.  Every core-1 case of tests/train_core_cases.py (self and cross: 1 .. 64 items, 65 .. 256, one 1024-item case per geometry,
nq = 1, item-major keys, every special-block position) through d4_train_attn_core_bf16 / d4_train_xattn_core_bf16 against the exact float64
reference of tests/train_core_ref.py, within 2 x E16[family][tensor] (tests/train_bf16_core_ref.py: the error of the contract's emulation,
measured and asserted by tests/test_train_attn_bf16_host.py), with all the ownership checks of tests/test_gpu_train_cores.py (whose SelfCall /
CrossCall run the calls, on a shim that substitutes the two entries and size queries): NaN-pattern guards behind every buffer and behind the
planes, pad columns untouched, +0.0 mix column without residuals, inputs unchanged, the forward-only call with the same o3 bits and no
gradient written, two calls with the same bits; the form recorded under the new families, which list exactly their 6 + 3 forms while the old
families still list 13 + 6.  The fp32 entries at core 1 do not follow d4_train_attn_products_set (same bits, guard behind their planes intact
with the switch at 1).  The refusals return non-zero, write nothing and name the argument.

Blocks.  trunk_ops.time_attention / space_attention / cross_attention with `attn_products='bf16'` against the float64 oracle
(oracle/restate.py) evaluated twice on the CPU: as is, and with restate.attend wrapped here so that q, k', v', p, dO and dS are rounded to
bf16 wherever a side exceeds 64 items (straight-through rounding of values, a gradient-rounding identity).  D_emu is the distance of the two
per tensor, the bound 3 x D_emu + 2e-4 (DESIGN.md 8's scheme with the fp32 block tests' tolerance).  Each result differs from the 'fp32'
call; at <= 64 items the two are bit-identical (under a d4_debug_switch hook the short problem takes the bf16 form instead); every call
puts the switch back.

Model.  DynamicsWorldModel(train_attn_products='bf16') on wide frames (77 tokens, 72 latents) and on a 66-frame clip, losses and gradients
against the oracle at 3 x D_emu plus the fp32 model tests' tolerances; a model whose attentions stay <= 64 is bit-identical with the option on
and off; with train_matmul_dtype='bf16' a step is finite and reproducible bit for bit.

Measured on the MI355X (135 tests, 4.9 s): the largest error / bound of the operator cases is 0.40 for every tensor of both families (the
kernels land on the emulation's own error to three digits: 0.40 = 1 / (2 x 1.25)); the blocks' distances are 0.83 .. 1.30 x D_emu (D_emu
1.4e-3 .. 1.1e-2; the bound is 3 x D_emu + 2e-4); the models' largest distance / bound is 0.56 (77-token frames, 129 gradients) and 0.36 (66
frames, 113 gradients)."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import bf16_emulation as emu
import test_gpu_long_clips as LC
import test_gpu_train_cores as T
import test_gpu_wide_frames as WFG
import train_bf16_core_ref as B
import train_core_cases as K
import train_core_ref as R
import wide_frames_cases as WC
from dreamer4_amd import _lib
from oracle import restate

pytestmark = pytest.mark.gpu

SELF1 = [c for c in K.SELF if c['core'] == 1]
CROSS1 = [c for c in K.CROSS if c['core'] == 1]
SEEN = {'train_attn_bf16': set(), 'train_xattn_bf16': set()}
REPEATED = set()
WORST = {}                       # (family, tensor) -> (error / bound, case)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


class Bf16Entries:
    """The library as SelfCall / CrossCall of test_gpu_train_cores use it, with the two entries and size queries of the bf16 form in place of
    the fp32 ones (the bf16 size queries take the items per problem, which the case knows)."""
    def __init__(self, lib, c):
        self._lib, self._c = lib, c

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def d4_train_attn_core(self, *a):
        return self._lib.d4_train_attn_core_bf16(*a)

    def d4_train_xattn_core(self, *a):
        return self._lib.d4_train_xattn_core_bf16(*a)

    def d4_train_attn_core_plane_floats(self, rows, heads, dh):
        assert rows == self._c['groups'] * self._c['items']
        return self._lib.d4_train_attn_core_bf16_plane_floats(self._c['groups'], self._c['items'], heads, dh)

    def d4_train_xattn_core_plane_floats(self, q_rows, k_rows, heads, dh):
        c = self._c
        assert (q_rows, k_rows) == (c['groups'] * c['nq'], c['groups'] * c['nk'])
        return self._lib.d4_train_xattn_core_bf16_plane_floats(c['groups'], c['nq'], c['nk'], heads, dh)


def bf16_form(c):
    return c['form'].replace('tiled<', 'tiled_bf16<')


def last_form(lib, family):
    f = lib.d4_debug_last_form(family.encode())
    assert f is not None, f'no {family} form recorded'
    SEEN[family].add(f.decode())
    return f.decode()


def check_values(c, got, ref):
    fam = B.family(c)
    bad = {}
    for n, (e, et) in R.errors(got, ref).items():
        bound = B.bound(fam, n)
        print(f"{c['name']} {n}: err {e:.3e} per problem, {et:.3e} per tensor (bound {bound:.3e})")
        if e / bound > WORST.get((fam, n), (0., ''))[0]:
            WORST[(fam, n)] = (e / bound, c['name'])
        if not e <= bound:
            bad[n] = (e, bound)
    assert not bad, f"{c['name']}: above the bound: {bad}"


# ------------------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize('c', SELF1, ids=[c['name'] for c in SELF1])
def test_self_core_bf16(lib, c):
    call = T.SelfCall(Bf16Entries(lib, c), c)
    hd, H, rows = call.hd, c['heads'], call.rows
    rc, o = call()
    assert rc == 0, lib.d4_last_error().decode()
    assert last_form(lib, 'train_attn_bf16') == bf16_form(c)
    hp4 = R.hp4_of(H)
    T.check_owned('dproj', o['dproj'], rows, call.ldp, T.owned_columns(call.ldp, [(0, 3 * hd + H), (3 * hd + hp4, 3 * hd + hp4 + H)]))
    T.check_owned('o3', o['o3'], rows, hd, T.owned_columns(hd, [(0, hd)]))
    T.check_owned('d_rv', o['d_rv'], rows, hd, T.owned_columns(hd, [(0, hd)] if c['vres'] else []))
    T.check_owned('dgamma_part', o['dgamma'], c['groups'], hd, T.owned_columns(hd, [(0, hd)]))
    assert T.pat(o['planes'][call.pf:]).all(), 'the guard behind the planes was written'
    if not c['vres']:
        mix = o['dproj'].cpu()[:rows * call.ldp].view(rows, call.ldp)[:, 3 * hd + hp4:3 * hd + hp4 + H]
        assert (mix.contiguous().view(torch.int32) == 0).all(), 'the mix-logit gradient without residuals is not +0.0'
    call.inputs_unchanged()
    check_values(c, call.gather(o), K.expect(c))
    rc, f = call(backward=False)
    assert rc == 0, lib.d4_last_error().decode()
    assert T.same_bits(f['o3'], o['o3']), 'the forward-only o3 differs from the o3 of the forward-and-backward call'
    for n in ('dproj', 'd_rv', 'dgamma'):
        assert T.pat(f[n]).all(), f'the forward-only call wrote {n}'
    if bf16_form(c) not in REPEATED:
        REPEATED.add(bf16_form(c))
        rc, o2 = call()
        assert rc == 0
        for n in ('o3', 'dproj', 'd_rv', 'dgamma'):
            assert T.same_bits(o[n], o2[n]), f'{n}: two calls differ'


@pytest.mark.parametrize('c', CROSS1, ids=[c['name'] for c in CROSS1])
def test_cross_core_bf16(lib, c):
    call = T.CrossCall(Bf16Entries(lib, c), c)
    hd, H = call.hd, c['heads']
    rc, o = call()
    assert rc == 0, lib.d4_last_error().decode()
    assert last_form(lib, 'train_xattn_bf16') == bf16_form(c)
    T.check_owned('dprojq', o['dprojq'], call.rq, call.ldq, T.owned_columns(call.ldq, [(0, hd + H)]))
    T.check_owned('dprojk', o['dprojk'], call.rk, call.ldk, T.owned_columns(call.ldk, [(0, 2 * hd)]))
    T.check_owned('o3', o['o3'], call.rq, hd, T.owned_columns(hd, [(0, hd)]))
    T.check_owned('dgamma_part', o['dgamma'], c['groups'], hd, T.owned_columns(hd, [(0, hd)]))
    assert T.pat(o['planes'][call.pf:]).all(), 'the guard behind the planes was written'
    call.inputs_unchanged()
    check_values(c, call.gather(o), K.expect(c))
    rc, f = call(backward=False)
    assert rc == 0, lib.d4_last_error().decode()
    assert T.same_bits(f['o3'], o['o3']), 'the forward-only o3 differs from the o3 of the forward-and-backward call'
    for n in ('dprojq', 'dprojk', 'dgamma'):
        assert T.pat(f[n]).all(), f'the forward-only call wrote {n}'
    if bf16_form(c) not in REPEATED:
        REPEATED.add(bf16_form(c))
        rc, o2 = call()
        assert rc == 0
        for n in ('o3', 'dprojq', 'dprojk', 'dgamma'):
            assert T.same_bits(o[n], o2[n]), f'{n}: two calls differ'


@pytest.mark.parametrize('key', ['frame-dh32-n33', 'time-dh64-n100', 'cross-4x256-dh16', 'cross-3x20-dh32'])
def test_the_fp32_entries_do_not_follow_the_switch(lib, key):
    """d4_train_attn_core / d4_train_xattn_core at core 1 with d4_train_attn_products_set(1) in force: the fp32 form on planes of the fp32 size
    (the bf16 images would not fit behind them) — the bits of the call with the switch at 0, the guard behind the planes intact, the form
    recorded under the old family and nothing under the new one."""
    cross = key.startswith('cross')
    c = next(c for c in (CROSS1 if cross else SELF1) if c['key'] == key)
    call = (T.CrossCall if cross else T.SelfCall)(lib, c)
    fam, fam16 = ('train_xattn', 'train_xattn_bf16') if cross else ('train_attn', 'train_attn_bf16')
    names = ('o3', 'dprojq', 'dprojk', 'dgamma') if cross else ('o3', 'dproj', 'd_rv', 'dgamma')
    rc, off = call()
    assert rc == 0, lib.d4_last_error().decode()
    before = lib.d4_debug_last_form(fam16.encode())
    assert lib.d4_train_attn_products_set(1) == 0
    try:
        rc, on = call()
        form, after = lib.d4_debug_last_form(fam.encode()).decode(), lib.d4_debug_last_form(fam16.encode())
        rc_short, short = call(pf=call.pf - 1)
    finally:
        assert lib.d4_train_attn_products_set(0) == 1
    assert rc == 0, lib.d4_last_error().decode()
    assert form == c['form'] and after == before
    for n in names:
        assert T.same_bits(off[n], on[n]), f'{n}: the switch changed the bits of the fp32 entry'
    assert T.pat(on['planes'][call.pf:]).all(), 'the guard behind the planes was written with the switch at 1'
    assert rc_short != 0 and all(T.pat(short[n]).all() for n in names)


REFUSALS = [(dict(core=0), 'core 0'), (dict(planes=None), 'planes'), (dict(pf='need-1'), 'plane_floats'), (dict(dh=48), 'dim_head')]


@pytest.mark.parametrize('over,frag', REFUSALS + [(dict(items=1025), 'items')], ids=lambda v: '-'.join(v) if isinstance(v, dict) else None)
def test_self_core_bf16_refusals(lib, over, frag):
    c = next(c for c in SELF1 if c['key'] == 'frame-dh32-n32')
    call = T.SelfCall(Bf16Entries(lib, c), c)
    over = dict(over)
    if over.get('pf') == 'need-1':
        over['pf'] = call.pf - 1
    rc, o = call(**over)
    assert rc != 0, f'{over} was accepted'
    err = lib.d4_last_error().decode()
    assert frag in err and 'd4_train_attn_core_bf16' in err, err
    if 'core' in over:
        assert 'no bf16 form' in err, err
    for n in ('o3', 'dproj', 'd_rv', 'dgamma'):
        assert T.pat(o[n]).all(), f'a refused call wrote {n}'
    assert T.pat(o['planes']).all(), 'a refused call wrote the planes'


@pytest.mark.parametrize('over,frag', REFUSALS + [(dict(nq=1025), 'nq'), (dict(nk=1025), 'nk')], ids=lambda v: '-'.join(v) if isinstance(v, dict) else None)
def test_cross_core_bf16_refusals(lib, over, frag):
    c = next(c for c in CROSS1 if c['key'] == 'cross-3x20-dh32')
    call = T.CrossCall(Bf16Entries(lib, c), c)
    over = dict(over)
    if over.get('pf') == 'need-1':
        over['pf'] = call.pf - 1
    rc, o = call(**over)
    assert rc != 0, f'{over} was accepted'
    err = lib.d4_last_error().decode()
    assert frag in err and 'd4_train_xattn_core_bf16' in err, err
    if 'core' in over:
        assert 'no bf16 form' in err, err
    for n in ('o3', 'dprojq', 'dprojk', 'dgamma'):
        assert T.pat(o[n]).all(), f'a refused call wrote {n}'
    assert T.pat(o['planes']).all(), 'a refused call wrote the planes'


def _forms(lib, fam):
    n = lib.d4_debug_forms(fam.encode(), 0, None)
    out = set()
    for i in range(n):
        s = C.c_char_p()
        assert lib.d4_debug_forms(fam.encode(), i, C.byref(s)) == n
        out.add(s.value.decode())
    assert len(out) == n
    return out


def test_every_form_of_the_two_new_families_was_seen(lib):
    want = {'train_attn_bf16': {f'tiled_bf16<{g},{dh}>' for g in ('time', 'frame') for dh in (64, 32, 16)},
            'train_xattn_bf16': {f'tiled_bf16<cross,{dh}>' for dh in (64, 32, 16)}}
    for fam, forms in want.items():
        assert _forms(lib, fam) == forms
        assert SEEN[fam] == forms, f'{fam}: never launched {sorted(forms - SEEN[fam])}'
        assert forms <= REPEATED
    assert len(_forms(lib, 'train_attn')) == 13 and len(_forms(lib, 'train_xattn')) == 6
    assert not any('bf16' in f for f in _forms(lib, 'train_attn') | _forms(lib, 'train_xattn'))
    for (fam, n), (e, name) in sorted(WORST.items()):
        print(f'largest error / bound: {fam} {n}: {e:.3f} ({name})')


# ------------------------------------------------------------------------------------------------------------------- the oracle's emulation
def _st(x):
    """straight-through rounding of the values"""
    return x + (x.detach().to(torch.bfloat16).to(x.dtype) - x.detach())


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to bf16"""
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


@contextlib.contextmanager
def bf16_attend():
    """restate.attend with the roundings of the bf16 form wherever the blocks take the tiled core (a side above 64 items): q, k', v' and p
    rounded (values), dO and dS rounded (gradients); everything else, and every attention of at most 64 items, as the oracle has it."""
    orig = restate.attend

    def attend(q, k, v, softclamp_value=None, mask=None, causal=False):
        if max(q.shape[-2], k.shape[-2]) <= 64:
            return orig(q, k, v, softclamp_value=softclamp_value, mask=mask, causal=causal)
        q, k, v = _st(q), _st(k), _st(v)
        sim = _RoundGrad.apply(torch.einsum('bhid,bhjd->bhij', q, k)) * q.shape[-1] ** -0.5
        if softclamp_value is not None:
            sim = restate.softclamp(sim, softclamp_value)
        neg = -torch.finfo(sim.dtype).max
        if mask is not None:
            sim = sim.masked_fill(~mask, neg)
        if causal:
            i, j = sim.shape[-2:]
            sim = sim.masked_fill(torch.ones((i, j), dtype=torch.bool).triu(j - i + 1), neg)
        return _RoundGrad.apply(torch.einsum('bhij,bhjd->bhid', _st(sim.softmax(dim=-1)), v))

    restate.attend = attend
    try:
        yield
    finally:
        restate.attend = orig


def _clone(d):
    return {k: v.detach().clone() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _emulated(kind, shape):
    run = {'time': LC._oracle_run, 'space': WC.space_oracle_run, 'cross': WC.cross_oracle_run}[kind]
    with bf16_attend():
        return _clone(run(shape))


def _block_check(kind, shape, got, fp32):
    ref = {'time': LC._oracle, 'space': WC.space_oracle, 'cross': WC.cross_oracle}[kind](shape)
    emul = _emulated(kind, shape)
    assert set(got) == set(ref)
    bad, differs = [], 0
    for k in ref:
        d_emu, d = emu.scaled_max(emul[k], ref[k]), emu.scaled_max(got[k], ref[k])
        print(f'  {kind} {shape[:3]} {k}: {d:.3e}  (D_emu {d_emu:.3e}, bound {3 * d_emu + 2e-4:.3e})')
        if not d <= 3 * d_emu + 2e-4:
            bad.append((k, d, d_emu))
        differs += not torch.equal(got[k], fp32[k])
    assert not bad, bad
    assert differs >= len(ref) - 1, 'the option left no trace: the block ran its fp32 products'
    assert _lib.load().d4_train_attn_products_set(0) == 0, 'a call left the switch on'


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('shape', LC.LONG[:4])
def test_long_time_attention_bf16_products_vs_oracle(shape, save_forward, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    _block_check('time', shape, LC._gpu(shape, attn_products='bf16'), LC._gpu(shape, attn_products='fp32'))


def test_wide_space_attention_bf16_products_vs_oracle():
    shape = WC.SPACE_WIDE[2]                                                # 130 tokens, 4 specials across the 128 boundary
    _block_check('space', shape, WFG._space_gpu(shape, wide=True, attn_products='bf16'), WFG._space_gpu(shape, wide=True))


def test_wide_cross_attention_bf16_products_vs_oracle():
    shape = (3, 4, 256, 128, 8, 3, 16, True, True, 5.)                      # nq 4, nk 256, item-major keys
    _block_check('cross', shape, WFG._cross_gpu(shape, wide=True, attn_products='bf16'), WFG._cross_gpu(shape, wide=True))


def test_the_option_leaves_no_trace_up_to_64_items(lib):
    runs = ((LC._gpu, LC.SHORT[3], {}), (WFG._space_gpu, WC.SPACE_SHORT[5], dict(wide=True)), (WFG._cross_gpu, WC.CROSS_SHORT[1], dict(wide=True)),
            (WFG._space_gpu, WC.SPACE_WIDE[0], {}))
    for run, shape, kw in runs[:3]:
        a, b = run(shape, attn_products='fp32', **kw), run(shape, attn_products='bf16', **kw)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)
    with pytest.raises(_lib.D4Error, match='items per group'):             # the option does not widen anything by itself
        runs[3][0](runs[3][1], attn_products='bf16')
    assert lib.d4_train_attn_products_set(0) == 0 and lib.d4_train_wide_set(0) == 0


@pytest.mark.parametrize('hook,fam,run,shape,kw', [
    (b'time_attn_tiled', 'train_attn_bf16', LC._gpu, LC.SHORT[3], {}),
    (b'space_attn_tiled', 'train_attn_bf16', WFG._space_gpu, WC.SPACE_SHORT[5], {}),
    (b'cross_attn_tiled', 'train_xattn_bf16', WFG._cross_gpu, WC.CROSS_SHORT[1], {})], ids=['time', 'space', 'cross'])
def test_under_its_hook_a_short_problem_takes_the_bf16_form(lib, hook, fam, run, shape, kw):
    """At <= 64 items the tiled core runs only under its test hook; with the option it is then the bf16 form: the form is recorded, the
    result differs from the hooked fp32 call and stays close to it (3e-2 of scale: bf16 products against fp32 ones)."""
    assert lib.d4_debug_switch(hook, 1) == 0
    try:
        a = run(shape, attn_products='fp32', **kw)
        b = run(shape, attn_products='bf16', **kw)
        form = lib.d4_debug_last_form(fam.encode()).decode()
    finally:
        assert lib.d4_debug_switch(hook, 0) == 1
    assert form.startswith('tiled_bf16<' + {b'time_attn_tiled': 'time', b'space_attn_tiled': 'frame', b'cross_attn_tiled': 'cross'}[hook]), form
    for k in a:
        assert not torch.equal(a[k], b[k]), k
        assert emu.scaled_max(b[k], a[k]) <= 3e-2, (k, emu.scaled_max(b[k], a[k]))
    assert lib.d4_train_attn_products_set(0) == 0


def test_the_option_is_refused_on_the_dispatcher_route(monkeypatch):
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', '1')
    with pytest.raises(NotImplementedError, match='attn_products'):
        LC._gpu(LC.LONG[0], attn_products='bf16')
    with pytest.raises(ValueError, match='fp8'):
        LC._gpu(LC.LONG[0], attn_products='fp8')


# ------------------------------------------------------------------------------------------------------------------- the model
def _model_run(m, cfg, W, lat, actions, step_log2, sig, noise):
    """the oracle's flow + shortcut losses and the gradients of their sum, in fp32 as the model tests this follows"""
    own = dict(m.named_parameters())
    Wd = {k: (v.clone().requires_grad_() if k in own and v.is_floating_point() else v) for k, v in W.items()}
    fl, sl = restate.dynamics_flow_losses(cfg, Wd, lat, noise, sig, step_log2, True, actions=actions)
    (fl + sl).backward()
    out = {'loss/flow': fl.detach(), 'loss/shortcut': sl.detach()}
    out.update({'grad/' + k: v.grad for k, v in Wd.items() if v.requires_grad and v.grad is not None})
    return out


def _model_gpu(m, lat, actions, step_log2, sig, noise):
    m.zero_grad(set_to_none=True)
    draws = dict(shortcut_train=True, step_sizes_log2=step_log2, signal_levels=sig, noise=noise)
    total, (fl, sl, *_) = m(latents=lat, discrete_actions=actions, return_all_losses=True, draws=draws, add_autoregressive_action_loss=False)
    total.backward()
    torch.cuda.synchronize()
    out = {'loss/flow': fl.detach().cpu(), 'loss/shortcut': sl.detach().cpu()}
    out.update({'grad/' + k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None})
    return out


def _model_check(m, cfg, W, inputs):
    ref = _model_run(m, cfg, W, *inputs)
    with bf16_attend():
        emul = _model_run(m, cfg, W, *inputs)
    m = m.cuda()
    assert m.train_attn_products == 'bf16'
    got = _model_gpu(m, *inputs)
    m.train_attn_products = 'fp32'
    fp32 = _model_gpu(m, *inputs)
    m.train_attn_products = 'bf16'
    bad, n, differs = [], 0, 0
    for k in ref:
        assert k in got, k
        assert torch.isfinite(got[k]).all(), k
        d_emu, d = emu.scaled_max(emul[k], ref[k]), emu.scaled_max(got[k], ref[k])
        tol = 1e-5 if k.startswith('loss/') else 1e-3
        n += k.startswith('grad/')
        differs += not torch.equal(got[k], fp32[k])
        if not d <= 3 * d_emu + tol:
            bad.append((k, d, d_emu))
    worst = max(((emu.scaled_max(got[k], ref[k]) / (3 * emu.scaled_max(emul[k], ref[k]) + 1e-3), k) for k in ref if k.startswith('grad/')))
    print(f'\n{n} gradients; largest distance / bound {worst[0]:.3f} ({worst[1]}); flow {got["loss/flow"].item():.8f} (oracle {ref["loss/flow"].item():.8f})')
    assert not bad, bad
    assert n >= 90 and differs >= n // 2, 'the option left no trace: the model ran its fp32 products'
    assert _lib.load().d4_train_attn_products_set(0) == 0
    return m, got


def test_world_model_bf16_products_on_77_token_frames_vs_oracle():
    from dreamer4_amd import DynamicsWorldModel
    from util import oracle_config, randomize_weights
    torch.manual_seed(5)
    m = randomize_weights(DynamicsWorldModel(**WFG.WM_KW, train_wide_frames=True, train_attn_products='bf16'))
    cfg = oracle_config(m)
    W = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _model_check(m, cfg, W, WFG._wm_inputs(m, 1, 3))


def test_world_model_bf16_products_on_a_66_frame_clip_vs_oracle():
    from dreamer4_amd import DynamicsWorldModel
    from util import oracle_config, randomize_weights
    torch.manual_seed(6)
    m = randomize_weights(DynamicsWorldModel(**LC.TRUNK_KW, train_attn_products='bf16'))
    assert m.train_wide_frames is False
    cfg = oracle_config(m)
    W = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _model_check(m, cfg, W, WFG._wm_inputs(m, 1, 66))


def test_a_model_whose_attentions_stay_small_is_bit_identical_with_the_option():
    from dreamer4_amd import DynamicsWorldModel
    from util import randomize_weights
    torch.manual_seed(6)
    m = randomize_weights(DynamicsWorldModel(**LC.TRUNK_KW, train_attn_products='bf16')).cuda()
    inputs = WFG._wm_inputs(m, 2, 9)
    on = _model_gpu(m, *inputs)
    m.train_attn_products = 'fp32'
    off = _model_gpu(m, *inputs)
    assert set(on) == set(off) and len(on) >= 90
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_bf16_products_with_bf16_linears_one_step_finite_and_reproducible():
    from dreamer4_amd import DynamicsWorldModel
    from util import randomize_weights
    torch.manual_seed(6)
    m = randomize_weights(DynamicsWorldModel(**LC.TRUNK_KW, train_attn_products='bf16', train_matmul_dtype='bf16')).cuda()
    inputs = WFG._wm_inputs(m, 1, 66)
    a, b = _model_gpu(m, *inputs), _model_gpu(m, *inputs)
    m.train_attn_products = 'fp32'
    c = _model_gpu(m, *inputs)
    assert set(a) == set(b) and len(a) >= 90
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    assert sum(not torch.equal(a[k], c[k]) for k in a) >= len(a) // 2, 'the option left no trace beside the bf16 Linears'
    lib = _lib.load()
    assert lib.d4_train_attn_products_set(0) == 0 and lib.d4_train_arith_set(0) == 0
