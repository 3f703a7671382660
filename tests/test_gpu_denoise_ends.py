"""GPU: the latent-token ends of a denoise evaluation (csrc/latent_ends.hip and the engine rules around it).

Three changes of the fp32 dynamics engine, each behind a d4_debug_switch hook (default 1; 0 restores the launches it replaces), each bit-identical
to the path it replaces:
  lqap_in_fused         latents -> K | V projection -> learned-query attention in one per-frame kernel (e->lkv is not written);
  lqap_out_fused        learned-query attention -> latent prediction in one per-frame kernel (e->oatt is not written);
  last_layer_compact_q  the last layer's q | head-gate columns are projected on the compact rows only (two problems of one pair launch).

Operator tests: d4_lqap_in / d4_lqap_out against the launches they replace (d4_gemm, d4_small_attn) with torch.equal, and against a float64
reference at the bound tests/test_gpu_attn_cores.py holds the attn_mfma forms to (BOUND['small_attn'] x max |float64|).  The fused kernels carry
the bits of the LDS-DMA GEMM family (csrc/gemm2.hip), which is what the dispatcher runs at the frame counts the engine's rule admits (>= 192); at
1 and 3 frames the dispatcher would take the few-row kernel (another k order), so there the chain's d4_gemm is pinned to that family with
d4_gemm_force_config — every configuration of the family gives the same bits.

Rollout tests: every hook alone and all together against all off, torch.equal on every tensor of the Experience and on the time cache."""
import ctypes as C

import pytest
import torch

import attn_core_cases as K
from attn_core_ref import small_attn_ref
from dreamer4_amd import _lib
from util import make_noise, oracle_config, randomize_weights, small_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOKS = (b'lqap_in_fused', b'lqap_out_fused', b'last_layer_compact_q')
H, DH, HD = 8, 64, 512
EPS = 1.1920928955078125e-07
BOUND = K.BOUND['small_attn']
FRAMES = (1, 3, 200)
SHAPES = ((32, 4, 32), (17, 3, 32), (16, 1, 64))           # (n, ns, dl): ragged second key / query tile, a single query, a two-k-tile projection
V2_32x64 = 106                                             # d4_gemm_force_config: configuration 6 of the LDS-DMA family


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(g, *shape, scale=1.):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def gemm_chain(lib, frames, *args):
    """d4_gemm through the dispatcher where it takes the LDS-DMA family itself, pinned to that family at the few-row frame counts"""
    pin = frames < 192
    if pin:
        lib.d4_gemm_force_config(V2_32x64)
    try:
        _lib.check(lib.d4_gemm(*args))
    finally:
        if pin:
            lib.d4_gemm_force_config(-1)


# ------------------------------------------------------------------------------------------------------------------ operators
@pytest.fixture(scope='module', params=[(f, s) for f in FRAMES for s in SHAPES], ids=lambda p: f'f{p[0]}-n{p[1][0]}-ns{p[1][1]}-dl{p[1][2]}')
def lqap_in_case(request, lib):
    frames, (n, ns, dl) = request.param
    g = torch.Generator().manual_seed(1000 * frames + n)
    lat = rnd(g, frames * n, dl)
    lat[1 % (frames * n)] = 0.                              # an all-zero latent row: the eps path of the row scale
    w = rnd(g, 2 * HD, dl, scale=dl ** -0.5)
    q, gate, gamma = rnd(g, ns, HD), rnd(g, ns, H), rnd(g, HD, scale=0.2)
    kv = torch.full((frames * n, 2 * HD), float('nan'), device=DEV)
    chain = torch.full((frames * ns, HD), float('nan'), device=DEV)
    gemm_chain(lib, frames, _lib.ptr(lat), dl, _lib.ptr(w), dl, _lib.ptr(kv), 2 * HD, None, None, 0, frames * n, 2 * HD, dl, _lib.GEMM_RMS_ROWSCALE, EPS, stream())
    vp = C.c_void_p(kv.data_ptr() + 4 * HD)
    _lib.check(lib.d4_small_attn(_lib.ptr(q), 0, HD, _lib.ptr(kv), n * 2 * HD, 2 * HD, vp, n * 2 * HD, 2 * HD, _lib.ptr(gate), 0, H, _lib.ptr(gamma),
                                 None, 0, 0, None, 0, 0, _lib.ptr(chain), ns * HD, HD, None, frames, H, ns, n, 0., 0, 0, 0, 0, 1, DH, stream()))
    fused = torch.full((frames * ns, HD), float('nan'), device=DEV)
    _lib.check(lib.d4_lqap_in(_lib.ptr(lat), dl, _lib.ptr(w), dl, _lib.ptr(q), _lib.ptr(gate), _lib.ptr(gamma), _lib.ptr(fused), frames, H, n, ns, dl, EPS, stream()))
    torch.cuda.synchronize()
    # float64 reference of the same operation
    x = lat.double().cpu()
    xs = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS)
    kv64 = (xs @ w.double().cpu().T).view(frames, n, 2, H, DH)
    k64, v64 = kv64[:, :, 0].transpose(1, 2), kv64[:, :, 1].transpose(1, 2)
    ref = small_attn_ref(q.cpu().view(1, ns, H, DH).transpose(1, 2), k64, v64, gamma.cpu().view(H, DH), gate.cpu().T[None], clamp=0.)
    ref = ref.transpose(1, 2).reshape(frames * ns, HD)
    return dict(chain=chain.cpu(), fused=fused.cpu(), ref=ref, kv=kv.cpu())


def test_lqap_in_is_bitwise_the_gemm_then_attention_chain(lqap_in_case):
    c = lqap_in_case
    assert not torch.isnan(c['chain']).any() and not torch.isnan(c['kv']).any()
    print(f"lqap_in vs chain: max abs diff {(c['fused'] - c['chain']).abs().max().item():.3e}")
    assert torch.equal(c['fused'], c['chain'])


def test_lqap_in_against_float64(lqap_in_case):
    c = lqap_in_case
    scale = c['ref'].abs().max().item()
    err = (c['fused'].double() - c['ref']).abs().max().item() / scale
    print(f'lqap_in vs float64: err {err:.3e} (bound {BOUND:.3e})')
    assert err <= BOUND


@pytest.fixture(scope='module', params=[(f, s) for f in FRAMES for s in SHAPES], ids=lambda p: f'f{p[0]}-n{p[1][0]}-ns{p[1][1]}-dl{p[1][2]}')
def lqap_out_case(request, lib):
    frames, (n, ns, dl) = request.param
    g = torch.Generator().manual_seed(2000 * frames + n)
    kv = rnd(g, frames * ns, 2 * HD)
    q, gate, gamma = rnd(g, n, HD), rnd(g, n, H), rnd(g, HD, scale=0.2)
    w = rnd(g, dl, HD, scale=HD ** -0.5)
    att = torch.full((frames * n, HD), float('nan'), device=DEV)
    chain = torch.full((frames * n, dl), float('nan'), device=DEV)
    vp = C.c_void_p(kv.data_ptr() + 4 * HD)
    _lib.check(lib.d4_small_attn(_lib.ptr(q), 0, HD, _lib.ptr(kv), ns * 2 * HD, 2 * HD, vp, ns * 2 * HD, 2 * HD, _lib.ptr(gate), 0, H, _lib.ptr(gamma),
                                 None, 0, 0, None, 0, 0, _lib.ptr(att), n * HD, HD, None, frames, H, n, ns, 0., 0, 0, 0, 0, 1, DH, stream()))
    gemm_chain(lib, frames, _lib.ptr(att), HD, _lib.ptr(w), HD, _lib.ptr(chain), dl, None, None, 0, frames * n, dl, HD, 0, EPS, stream())
    fused = torch.full((frames * n, dl), float('nan'), device=DEV)
    _lib.check(lib.d4_lqap_out(_lib.ptr(kv), 2 * HD, _lib.ptr(q), _lib.ptr(gate), _lib.ptr(gamma), _lib.ptr(w), HD, _lib.ptr(fused), dl, frames, H, n, ns, dl, stream()))
    torch.cuda.synchronize()
    kv64 = kv.cpu().view(frames, ns, 2, H, DH)
    k64, v64 = kv64[:, :, 0].transpose(1, 2), kv64[:, :, 1].transpose(1, 2)
    o = small_attn_ref(q.cpu().view(1, n, H, DH).transpose(1, 2), k64, v64, gamma.cpu().view(H, DH), gate.cpu().T[None], clamp=0.)
    ref = o.transpose(1, 2).reshape(frames * n, HD) @ w.double().cpu().T
    return dict(chain=chain.cpu(), fused=fused.cpu(), ref=ref, att=att.cpu())


def test_lqap_out_is_bitwise_the_attention_then_gemm_chain(lqap_out_case):
    c = lqap_out_case
    assert not torch.isnan(c['chain']).any() and not torch.isnan(c['att']).any()
    print(f"lqap_out vs chain: max abs diff {(c['fused'] - c['chain']).abs().max().item():.3e}")
    assert torch.equal(c['fused'], c['chain'])


def test_lqap_out_against_float64(lqap_out_case):
    c = lqap_out_case
    scale = c['ref'].abs().max().item()
    err = (c['fused'].double() - c['ref']).abs().max().item() / scale
    print(f'lqap_out vs float64: err {err:.3e} (bound {BOUND:.3e})')
    assert err <= BOUND


def test_operators_refuse_what_they_cannot_run(lib):
    t = torch.zeros(4096, device=DEV)
    p = _lib.ptr(t)
    assert lib.d4_lqap_in(p, 48, p, 48, p, p, p, p, 1, H, 16, 4, 48, EPS, stream()) != 0         # dl % 32
    assert lib.d4_lqap_in(p, 32, p, 32, p, p, p, p, 1, H, 33, 4, 32, EPS, stream()) != 0         # n > 32
    assert lib.d4_lqap_out(p, 2 * HD, p, p, p, p, HD, p, 32, 1, H, 32, 17, 32, stream()) != 0    # ns > 16
    assert lib.d4_lqap_out(p, 2 * HD, p, p, p, p, HD, p, 32, 1, 4, 32, 4, 32, stream()) != 0     # heads


# ------------------------------------------------------------------------------------------------------------------ rollouts
class hooks:
    def __init__(self, *values):
        self.want = tuple(zip(HOOKS, values))

    def __enter__(self):
        lib = _lib.load()
        self.old = [(n, lib.d4_debug_switch(n, v)) for n, v in self.want]
        assert all(o in (0, 1) for _, o in self.old)

    def __exit__(self, *exc):
        lib = _lib.load()
        for n, o in self.old:
            lib.d4_debug_switch(n, o)


def tiny_model():
    return small_model(dim=64, depth=2, time_block_every=2, attn_heads=2, attn_dim_head=32, num_latent_tokens=4)


def wide_model(**kw):
    from dreamer4_amd import DynamicsWorldModel
    torch.manual_seed(0)
    return randomize_weights(DynamicsWorldModel(dim=512, dim_latent=32, num_latent_tokens=32, depth=2, num_discrete_actions=4, **kw), terminal_bias=-10.)


def time_last_model():
    return wide_model(time_block_every=2)


def heads16_model():
    """16 heads x 64: the fused projection has N = 3104 >= 2048 columns, which the default (split-operand) engine runs on the bf16 matrix cores
    (csrc/gemm_x3*.hip) — another arithmetic than the f32 pair launch, so the last layer's projection must stay one launch there"""
    return wide_model(attn_heads=16)


def heads16_mfma_model():
    """the same architecture with every GEMM on the f32-input MFMA: the whole projection is on the LDS-DMA family, the split applies"""
    return wide_model(attn_heads=16, matmul_dtype='fp32_mfma')


def fields(e):
    out = dict(latents=e.latents, agent_embed=e.agent_embed, rewards=e.rewards, values=e.values, log_probs=e.log_probs.discrete,
               unembeds=e.old_action_unembeds.discrete, actions=e.actions.discrete, lens=e.lens, terminals=e.terminals,
               is_truncated=e.is_truncated, episode_return=e.episode_return)
    assert all(torch.is_tensor(v) for v in out.values())
    return out


def kv_of(m, tc):
    return tc.kv().clone() if m.depth // m.time_block_every > 0 else torch.empty(0)


def engine_buffer(m, name, numel):
    """a writable view of an engine activation buffer (d4_debug_buffer)"""
    p = C.c_void_p()
    _lib.check(_lib.load().d4_debug_buffer(m._engine, name, C.byref(p)))
    off = p.value - m._ws.data_ptr()
    return m._ws[off:off + 4 * numel].view(torch.float32)


ARMS = {'off': (0, 0, 0), 'in': (1, 0, 0), 'out': (0, 1, 0), 'q': (0, 0, 1), 'on': (1, 1, 1)}
MODELS = {'dim512_b192': (wide_model, 192, 2), 'tiny': (tiny_model, 3, 3), 'time_last_b192': (time_last_model, 192, 2),
          'heads16_b192': (heads16_model, 192, 2), 'heads16_mfma_b192': (heads16_mfma_model, 192, 2)}
# which rules apply: (lqap_in / lqap_out: 8 heads x 64 and >= 192 frames; last_layer_compact_q: a space layer last, its projection on the LDS-DMA family)
APPLIES = {'dim512_b192': (True, True), 'time_last_b192': (True, False), 'heads16_b192': (False, False), 'heads16_mfma_b192': (False, True)}


@pytest.fixture(scope='module', params=list(MODELS))
def runs(request):
    """One model per shape, enqueued eagerly (the launch counter sees every kernel); the rollout per arm.  Before each rollout the buffers the
    fused paths leave alone are filled with NaN, and what is left of the NaN is recorded."""
    import os
    make, B, T = MODELS[request.param]
    old = os.environ.get('D4_GRAPH_MAX_ROWS')
    os.environ['D4_GRAPH_MAX_ROWS'] = '0'                  # read at engine creation
    try:
        m = make().cuda()
        nz = make_noise(oracle_config(m), T, B, 41)
        m.generate(1, batch_size=B, return_for_policy_optimization=True, noise={k: v[:1] for k, v in nz.items()})      # engine creation, weight preparation
    finally:
        if old is None:
            del os.environ['D4_GRAPH_MAX_ROWS']
        else:
            os.environ['D4_GRAPH_MAX_ROWS'] = old
    lib = _lib.load()
    out = {}
    for arm, values in list(ARMS.items()) * 2:             # twice: the first pass times the GEMM shapes each arm meets first, the second is what counts
        with hooks(*values):
            probes = {n: engine_buffer(m, n, 64) for n in (b'lkv', b'oatt', b'qc')}
            for v in probes.values():
                v.fill_(float('nan'))
            lib.d4_debug_switch(b'launch_count', 0)
            e, tc = m.generate(T, batch_size=B, return_for_policy_optimization=True, return_time_cache=True, noise=nz)
            torch.cuda.synchronize()
            count = lib.d4_debug_switch(b'launch_count', 0)
            out[arm] = dict(f=fields(e), kv=kv_of(m, tc), count=count, untouched={n: bool(torch.isnan(v).all()) for n, v in probes.items()})
    return dict(name=request.param, out=out, m=m, make=make)


def test_hooks_exist_and_default_on(lib):
    for n in HOOKS:
        assert lib.d4_debug_switch(n, 1) == 1


@pytest.mark.parametrize('arm', ['in', 'out', 'q', 'on'])
def test_every_hook_leaves_the_rollout_bitwise(runs, arm):
    a, b = runs['out']['off'], runs['out'][arm]
    for k in a['f']:
        assert torch.equal(a['f'][k], b['f'][k]), (arm, k)
    assert torch.equal(a['kv'], b['kv'])
    assert a['f']['latents'].abs().max().item() > 0


def test_rules_apply_where_they_should(runs):
    """Which path ran, from the launch counts and from the buffers only the replaced launches write."""
    o, name = runs['out'], runs['name']
    print(name, {k: (v['count'], v['untouched']) for k, v in o.items()})
    if name == 'tiny':                                     # 2 heads x 32, as many latents as spatial tokens: no rule applies — the same launches, nothing written
        assert len({v['count'] for v in o.values()}) == 1 and o['off']['count'] > 0
        assert all(v['untouched'] == {b'lkv': True, b'oatt': True, b'qc': True} for v in o.values())
        return
    ends, split = APPLIES[name]
    assert o['off']['untouched'] == {b'lkv': False, b'oatt': False, b'qc': True}          # all off: the replaced launches run, nothing writes e->qc
    for arm, buf in (('in', b'lkv'), ('out', b'oatt')):
        assert o[arm]['untouched'][buf] == ends and o['on']['untouched'][buf] == ends
        assert (o[arm]['count'] < o['off']['count']) == ends and o[arm]['count'] <= o['off']['count']
    assert o['q']['count'] == o['off']['count']           # (one pair launch in place of one launch)
    assert o['q']['untouched'][b'qc'] == (not split) and o['on']['untouched'][b'qc'] == (not split)


def test_every_configuration_of_the_lds_dma_family_gives_the_same_bits(lib):
    """What pinning the chain's d4_gemm to one configuration of the family relies on: the K | V projection at 3 frames under each of them."""
    g = torch.Generator().manual_seed(5)
    lat, w = rnd(g, 96, 32), rnd(g, 2 * HD, 32, scale=32 ** -0.5)
    outs = []
    for cfg in range(100, 100 + 10):
        kv = torch.full((96, 2 * HD), float('nan'), device=DEV)
        lib.d4_gemm_force_config(cfg)
        try:
            _lib.check(lib.d4_gemm(_lib.ptr(lat), 32, _lib.ptr(w), 32, _lib.ptr(kv), 2 * HD, None, None, 0, 96, 2 * HD, 32, _lib.GEMM_RMS_ROWSCALE, EPS, stream()))
        finally:
            lib.d4_gemm_force_config(-1)
        torch.cuda.synchronize()
        outs.append(kv.cpu())
    assert not torch.isnan(outs[0]).any()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_wm_forward_after_a_rollout_returns_the_same_prediction(runs):
    """d4_wm_forward wants every row of every layer: it keeps the single-launch projection, and its prediction is a fresh engine's bit for bit."""
    m = runs['m']
    cfg = oracle_config(m)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(4, 1, cfg.num_latent_tokens, cfg.dim_latent, generator=g)
    sig = torch.randint(0, cfg.max_steps, (4, 1), generator=g)
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4)
    with hooks(0, 0, 0):
        fresh = runs['make']().cuda()
        pred0, (agent0, _) = fresh(latents=lat, signal_levels=sig, step_sizes=4)
    assert torch.equal(pred, pred0) and torch.equal(agent, agent0)
    assert pred.abs().max().item() > 0


def test_eager_and_graph_replayed_frames_stay_bitwise_equal(monkeypatch):
    """All hooks on, 192 trajectories (every rule applies): enqueued eagerly and replayed from hipGraphs."""
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)
        m = wide_model().cuda()
        nz = make_noise(oracle_config(m), 3, 192, 3)
        e, tc = m.generate(3, batch_size=192, return_for_policy_optimization=True, return_time_cache=True, noise=nz)
        outs.append((fields(e), kv_of(m, tc)))
    (a, ka), (b, kb) = outs
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ka, kb)


def test_workspace_holds_the_new_buffers_and_the_learner_behind_them():
    """The regrouped projection image and the compact q buffer are part of the workspace's size: the learner's scratch, laid out behind them, is
    still inside it (a rollout followed by a learner step, as smoke())."""
    m = tiny_model().cuda()
    e = m.generate(3, batch_size=2, return_for_policy_optimization=True, noise=make_noise(oracle_config(m), 3, 2, 3))
    pl, vl = m.learn_from_experience(e, objective='ppo')
    assert torch.isfinite(pl).item() and torch.isfinite(vl).item()
