"""GPU: the register rows of a frame are a parameter — their share of the products that read slab 0 row by row is computed once.

Two changes of the fp32 dynamics engine, each behind a d4_debug_switch hook (default 1; 0 restores the full launches), each bit-identical:
  layer0_const_rows   layer 0's fused projection runs on the rows that change (from their dense image, row-mapped around the prefilled register rows);
  pool_const_keys     the in-loop pools' keys of slab 0 likewise: the changing rows for all pools in one batched row-mapped launch, and each pool's key
                      problem covers slabs 1 .. L - 1.

Operator tests: a row-mapped launch of each family that implements the map (d4_gemm_run_rowmap: the persistent split-operand kernel, the LDS-DMA family
single and batched) against the plain launch of the same product over the full matrix, torch.equal on the mapped rows, a NaN guard pattern left in the gap
rows; every other family refuses the map.

Engine tests (8 heads x 64: Nproj0 = 2064 selects the split-operand family; dim 128, depth 3: two in-loop pools; 2 spatial + 5 register tokens; B = 128 so
that a denoise evaluation has 128 x 9 = 1152 >= 1024 rows): each hook alone and both against both off, torch.equal on every output."""
import ctypes as C

import pytest
import torch

from dreamer4_amd import _lib
from util import make_noise, oracle_config, randomize_weights

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOKS = (b'layer0_const_rows', b'pool_const_keys')
ARMS = {'off': (0, 0), 'l0': (1, 0), 'ck': (0, 1), 'on': (1, 1)}
RMS = _lib.GEMM_RMS_ROWSCALE
EPS = 1.1920928955078125e-07
GUARD = 0x7FC12345                                          # a NaN bit pattern no kernel produces


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def guard(*shape):
    return torch.full(shape, GUARD, dtype=torch.int32, device=DEV).view(torch.float32)


def is_guard(t):
    return bool((t.view(torch.int32) == GUARD).all())


def mapped_rows(Md, Sc, S, lo, nr):
    r = torch.arange(Md)
    t = r % Sc
    return (r // Sc) * S + t + (t >= lo).long() * nr


def split_planes(lib, W):
    n = W.numel()
    plane = (n + 7) // 8 * 8
    W3 = torch.zeros(3 * plane, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.d4_split_bf16x3(_lib.ptr(W), _lib.ptr(W3), n, plane, stream()))
    return W3, plane


def desc(**f):
    d = _lib.GemmDesc()
    base = dict(rms_eps=EPS, batch=1, c2_last=1)
    base.update(f)
    for k, v in base.items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------------------------ operators
# (Md dense rows, Sc, S, lo, N, K): the last row tile is partly filled in every case; Md is no multiple of Sc in the first two (the last frame is cut short);
# a gap at the end of the frame (lo == Sc), in the middle, and right after row 0; more than one tile in both directions
MAPS = ((283, 4, 9, 3, 200, 64), (131, 3, 8, 3, 136, 32), (300, 10, 15, 5, 264, 96), (70, 2, 7, 1, 72, 32))


def operands(Md, Sc, S, lo, N, K, seed, batch=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    nr = S - Sc
    frames = (Md + Sc - 1) // Sc
    dense = torch.randn(Md, K, device=DEV, generator=g)
    dense[1] = 0.                                           # an all-zero row: the eps path of the row scale
    full = torch.randn(frames * S, K, device=DEV, generator=g)
    rows = mapped_rows(Md, Sc, S, lo, nr).to(DEV)
    full[rows] = dense
    W = torch.randn(batch * N, K, device=DEV, generator=g) / K ** 0.5
    bias = torch.randn(N, device=DEV, generator=g)
    return dense, full, rows, W, bias, frames, nr


@pytest.mark.parametrize('case', MAPS, ids=lambda c: 'x'.join(map(str, c)))
def test_row_mapped_split_operand_launch_is_the_plain_launch_on_the_mapped_rows(lib, case):
    Md, Sc, S, lo, N, K = case
    dense, full, rows, W, bias, frames, nr = operands(*case, seed=Md)
    W3, plane = split_planes(lib, W)
    plain = guard(frames * S, N)
    d = desc(A=dptr(full), lda=K, W=W3.data_ptr(), ldw=K, C=dptr(plain), ldc=N, bias=dptr(bias), M=frames * S, N=N, K=K, flags=RMS, Wb=W3.data_ptr(), wplane=plane)
    _lib.check(lib.d4_gemm_run(C.byref(d), _lib.GEMM_X3SK, 0, stream()))
    out = guard(frames * S, N)
    d = desc(A=dptr(dense), lda=K, W=W3.data_ptr(), ldw=K, C=dptr(out), ldc=N, bias=dptr(bias), M=Md, N=N, K=K, flags=RMS, Wb=W3.data_ptr(), wplane=plane)
    _lib.check(lib.d4_gemm_run_rowmap(C.byref(d), _lib.GEMM_X3SK, 0, Sc, S, lo, nr, stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(plain).any()
    assert torch.equal(out[rows], plain[rows])
    rest = torch.ones(frames * S, dtype=torch.bool, device=DEV)
    rest[rows] = False
    assert rest.sum().item() >= nr and is_guard(out[rest])   # the gap rows (and the cut-short last frame's missing rows) keep the guard


@pytest.mark.parametrize('cfg', [0, 2, 4, 6, 8])
@pytest.mark.parametrize('case', MAPS, ids=lambda c: 'x'.join(map(str, c)))
def test_row_mapped_lds_dma_launch_is_the_plain_launch_on_the_mapped_rows(lib, case, cfg):
    Md, Sc, S, lo, N, K = case
    dense, full, rows, W, bias, frames, nr = operands(*case, seed=Md + 1)
    plain, out = guard(frames * S, N), guard(frames * S, N)
    d = desc(A=dptr(full), lda=K, W=dptr(W), ldw=K, C=dptr(plain), ldc=N, bias=dptr(bias), M=frames * S, N=N, K=K, flags=RMS)
    _lib.check(lib.d4_gemm_run(C.byref(d), _lib.GEMM_V2, cfg, stream()))
    d = desc(A=dptr(dense), lda=K, W=dptr(W), ldw=K, C=dptr(out), ldc=N, bias=dptr(bias), M=Md, N=N, K=K, flags=RMS)
    _lib.check(lib.d4_gemm_run_rowmap(C.byref(d), _lib.GEMM_V2, cfg, Sc, S, lo, nr, stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(plain).any()
    assert torch.equal(out[rows], plain[rows])
    rest = torch.ones(frames * S, dtype=torch.bool, device=DEV)
    rest[rows] = False
    assert is_guard(out[rest])


@pytest.mark.parametrize('case', MAPS[:2], ids=lambda c: 'x'.join(map(str, c)))
def test_row_mapped_batched_lds_dma_launch(lib, case):
    """three members: one dense A (stride 0), the weights and the outputs at constant strides — the engine's batched key launch; no row scale on the second pass"""
    Md, Sc, S, lo, N, K = case
    nb = 3
    dense, full, rows, W, _, frames, nr = operands(*case, seed=Md + 2, batch=nb)
    for flags in (RMS, 0):
        plain, out = guard(nb, frames * S, N), guard(nb, frames * S, N)
        for b in range(nb):
            d = desc(A=dptr(full), lda=K, W=dptr(W, b * N * K), ldw=K, C=dptr(plain, b * frames * S * N), ldc=N, M=frames * S, N=N, K=K, flags=flags)
            _lib.check(lib.d4_gemm_run(C.byref(d), _lib.GEMM_V2, 6, stream()))
        d = desc(A=dptr(dense), lda=K, W=dptr(W), ldw=K, C=dptr(out), ldc=N, M=Md, N=N, K=K, flags=flags, batch=nb, strideA=0, strideW=N * K, strideC=frames * S * N)
        _lib.check(lib.d4_gemm_run_rowmap(C.byref(d), _lib.GEMM_V2, 6, Sc, S, lo, nr, stream()))
        torch.cuda.synchronize()
        assert not torch.isnan(plain).any()
        assert torch.equal(out[:, rows], plain[:, rows])
        rest = torch.ones(frames * S, dtype=torch.bool, device=DEV)
        rest[rows] = False
        assert is_guard(out[:, rest])


def test_a_family_without_the_row_map_refuses_it(lib):
    Sc, S, lo, N, K = 4, 9, 3, 136, 128
    nr = S - Sc

    def refused(family, cfg, Md=300, split=False, **kw):
        dense, full, rows, W, bias, frames, _ = operands(Md, Sc, S, lo, N, K, seed=9)
        out = guard(frames * S, N)
        f = dict(A=dptr(dense), lda=K, W=dptr(W), ldw=K, C=dptr(out), ldc=N, M=Md, N=N, K=K, flags=0)
        if split:
            W3, plane = split_planes(lib, W)
            f.update(W=W3.data_ptr(), Wb=W3.data_ptr(), wplane=plane)
        if kw.pop('res', False):
            kw.update(R=dptr(torch.zeros(frames * S, N, device=DEV)), ldr=N)
        smap = kw.pop('S_', S)
        f.update(kw)
        rc = lib.d4_gemm_run_rowmap(C.byref(desc(**f)), family, cfg, Sc, smap, lo, nr, stream())
        torch.cuda.synchronize()
        msg = lib.d4_last_error().decode()
        return rc != 0 and 'row map' in msg and is_guard(out)

    assert refused(_lib.GEMM_X3, 0, split=True)             # the plain split-operand kernel
    assert refused(_lib.GEMM_V2_KSPLIT, 0)
    assert refused(_lib.GEMM_SKINNY, 0, Md=40)
    assert refused(_lib.GEMM_TILE, 4)
    # the families that implement it, with an epilogue the map does not cover
    assert refused(_lib.GEMM_V2, 0, res=True)
    assert refused(_lib.GEMM_V2, 0, flags=_lib.GEMM_ACCUMULATE)
    assert refused(_lib.GEMM_X3SK, 0, split=True, flags=_lib.GEMM_SILU)
    assert refused(_lib.GEMM_V2, 0, S_=S + 1)               # a malformed map


# ------------------------------------------------------------------------------------------------------------------ engine
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


def make_model(**kw):
    from dreamer4_amd import DynamicsWorldModel
    torch.manual_seed(0)
    return randomize_weights(DynamicsWorldModel(dim=128, dim_latent=16, num_latent_tokens=8, depth=3, attn_heads=8, attn_dim_head=64, num_spatial_tokens=2,
                                                num_register_tokens=5, **kw), terminal_bias=-10.)


# no action token: 9 token rows (8 in a denoise evaluation: 128 x 8 = 1024 rows); one discrete action type, a time layer between two space layers; tasks +
# the action type with every layer a time layer (layer 0's time attention reads the reduced-form buffer; tokens never mix there, so the register columns
# show in the time cache alone, which every comparison includes)
VARIANTS = {'noaction': dict(kw=dict(time_block_every=3), tasks=False, act=False),
            'action': dict(kw=dict(num_discrete_actions=4, time_block_every=2), tasks=False, act=True),
            'tasks': dict(kw=dict(num_discrete_actions=4, num_tasks=3, time_block_every=1), tasks=True, act=True)}
B, T = 128, 3


def tasks_of(v, batch):
    return (torch.arange(batch) % 3) if v['tasks'] else None


def rollout(m, v, frames, batch, seed, **kw):
    """-> dict of every output tensor of the rollout and the time cache"""
    nz = make_noise(oracle_config(m), frames, batch, seed)
    if not v['act']:
        nz = dict(latent=nz['latent'], context=nz['context'], bern_u=nz['bern_u'])
        lat, tc = m.generate(frames, batch_size=batch, return_time_cache=True, noise=nz, tasks=tasks_of(v, batch), **kw)
        out = dict(latents=lat)
    else:
        e, tc = m.generate(frames, batch_size=batch, return_for_policy_optimization=True, return_time_cache=True, noise=nz, tasks=tasks_of(v, batch), **kw)
        out = dict(latents=e.latents, agent_embed=e.agent_embed, rewards=e.rewards, values=e.values, log_probs=e.log_probs.discrete,
                   unembeds=e.old_action_unembeds.discrete, actions=e.actions.discrete, lens=e.lens, terminals=e.terminals, episode_return=e.episode_return)
    out['kv'] = tc.kv().clone() if m.depth // m.time_block_every > 0 else torch.empty(0)
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in out.items()}


def forward(m, v, batch, frames, seed):
    cfg = oracle_config(m)
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(batch, frames, cfg.num_latent_tokens, cfg.dim_latent, generator=g)
    sig = torch.randint(0, cfg.max_steps, (batch, frames), generator=g)
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4, tasks=tasks_of(v, batch))
    torch.cuda.synchronize()
    return dict(pred=pred.clone(), agent=agent.clone())


def engine_buffer(m, name, numel, offset=0):
    p = C.c_void_p()
    _lib.check(_lib.load().d4_debug_buffer(m._engine, name, C.byref(p)))
    off = p.value - m._ws.data_ptr() + 4 * offset
    return m._ws[off:off + 4 * numel].view(torch.float32)


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)
    assert a[next(iter(a))].abs().max().item() > 0


def all_arms(m, v, run, probe=True):
    """run() under every arm; with `probe`, what is left of a NaN fill of the buffers only the full launches write"""
    lib = _lib.load()
    out = {}
    for arm, values in ARMS.items():
        with hooks(*values):
            probes = {}
            if probe:
                probes = {b'proj0': engine_buffer(m, b'proj0', 64), b'pool_kv': engine_buffer(m, b'pool_kv', 64, offset=5000 * 256)}
                for p in probes.values():
                    p.fill_(float('nan'))
            lib.d4_debug_switch(b'launch_count', 0)
            res = run()
            count = lib.d4_debug_switch(b'launch_count', 0)
            out[arm] = dict(res=res, count=count, untouched={n: bool(torch.isnan(p).all()) for n, p in probes.items()})
    return out


@pytest.fixture(scope='module', params=list(VARIANTS))
def eager(request):
    """One model per variant, enqueued eagerly (the launch counter sees every kernel).  A first pass of every arm lets each meet its GEMM shapes."""
    import os
    v = VARIANTS[request.param]
    old = os.environ.get('D4_GRAPH_MAX_ROWS')
    os.environ['D4_GRAPH_MAX_ROWS'] = '0'                  # read at engine creation
    try:
        m = make_model(**v['kw']).cuda()
        rollout(m, v, 1, B, 5)
    finally:
        if old is None:
            del os.environ['D4_GRAPH_MAX_ROWS']
        else:
            os.environ['D4_GRAPH_MAX_ROWS'] = old
    all_arms(m, v, lambda: rollout(m, v, T, B, 41), probe=False)
    return dict(name=request.param, v=v, m=m, rollout=all_arms(m, v, lambda: rollout(m, v, T, B, 41)))


def test_hooks_exist_and_default_on(lib):
    for n in HOOKS:
        assert lib.d4_debug_switch(n, 1) == 1


@pytest.mark.parametrize('arm', ['l0', 'ck', 'on'])
def test_every_hook_leaves_the_rollout_bitwise(eager, arm):
    same(eager['rollout']['off']['res'], eager['rollout'][arm]['res'], arm)


def test_the_reduced_forms_ran(eager):
    """From the buffers only the full launches write, and the launch counts: layer 0's projection is one launch either way, the keys add the batched one."""
    o = eager['rollout']
    print(eager['name'], {k: (a['count'], a['untouched']) for k, a in o.items()})
    assert o['off']['untouched'] == {b'proj0': False, b'pool_kv': False}
    assert o['l0']['untouched'] == {b'proj0': True, b'pool_kv': False}
    assert o['ck']['untouched'] == {b'proj0': False, b'pool_kv': True}
    assert o['on']['untouched'] == {b'proj0': True, b'pool_kv': True}
    evals = T * 5                                           # 4 denoise evaluations + the clean one per frame
    assert o['l0']['count'] == o['off']['count'] and o['ck']['count'] == o['off']['count'] + evals and o['on']['count'] == o['ck']['count']


def test_wm_forward_denoise_and_clean_rows_and_parallel_frames(eager):
    """d4_wm_forward (the clean layout: the agent row is one of the rows that change, with tasks) at one frame and at Tq = 3 parallel frames."""
    m, v = eager['m'], eager['v']
    for frames in (1, 3):
        forward(m, v, B, frames, 1)                        # (more parallel frames rebuild the engine and its workspace: before the probes are taken)
        o = all_arms(m, v, lambda: forward(m, v, B, frames, 7 + frames))
        for arm in ('l0', 'ck', 'on'):
            same(o['off']['res'], o[arm]['res'], (arm, frames))
        assert o['on']['untouched'][b'proj0'] and not o['off']['untouched'][b'proj0']
        if frames == 1:                                    # (at 3 frames the final pool's keys reach the probed rows of e->pool_kv)
            assert o['on']['untouched'][b'pool_kv'] and not o['off']['untouched'][b'pool_kv']


def test_prompt_pass_then_cached_decode_and_a_one_frame_call(eager):
    """A prompt of 2 frames: one parallel pass over Tq = 3 frames, then cached decode of the rest — the frame count changes between calls while the
    prefilled rows stay where every frame count finds them.  Then a call that generates a single frame."""
    m, v = eager['m'], eager['v']
    cfg = oracle_config(m)
    pl = torch.randn(B, 2, cfg.num_latent_tokens, cfg.dim_latent, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    kw = dict(prompt_latents=pl)
    if v['act']:
        kw['prompt_discrete_actions'] = torch.randint(0, 4, (B, 2), generator=torch.Generator().manual_seed(3))
    o = all_arms(m, v, lambda: rollout(m, v, 5, B, 11, **kw))
    for arm in ('l0', 'ck', 'on'):
        same(o['off']['res'], o[arm]['res'], (arm, 'prompt'))
    o = all_arms(m, v, lambda: rollout(m, v, 1, B, 12))
    for arm in ('l0', 'ck', 'on'):
        same(o['off']['res'], o[arm]['res'], (arm, 'one frame'))
    # a smaller batch in between writes its own slab blocks; the larger call after it still finds its constant rows
    a = rollout(m, v, 2, B // 2, 13)
    b = rollout(m, v, T, B, 41)
    with hooks(0, 0):
        same(rollout(m, v, 2, B // 2, 13), a, 'half batch')
        same(rollout(m, v, T, B, 41), b, 'after a half batch')
    same(b, eager['rollout']['off']['res'], 'against the first run')


def test_new_weights_give_new_constant_rows(eager):
    """`registers` and layer 0's weights change (in place: the engine prepares again): both on equals both off, and both differ from before."""
    m, v = eager['m'], eager['v']
    before = eager['rollout']['off']['res']
    saved = {k: p.detach().clone() for k, p in m.named_parameters()}
    try:
        with torch.no_grad():
            g = torch.Generator().manual_seed(77)
            for name, p in m.named_parameters():
                if name == 'register_tokens' or name.startswith('transformer.layers.0.') or name.startswith('transformer.attn_pools.'):
                    p.add_(torch.randn(p.shape, generator=g).to(p.device) * 0.05 * p.abs().mean())
        o = all_arms(m, v, lambda: rollout(m, v, T, B, 41))
        for arm in ('l0', 'ck', 'on'):
            same(o['off']['res'], o[arm]['res'], (arm, 'new weights'))
        assert o['on']['untouched'] == {b'proj0': True, b'pool_kv': True}
        assert not torch.equal(o['off']['res']['latents'], before['latents'])
    finally:
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(saved[k])
    same(rollout(m, v, T, B, 41), before, 'weights restored')


@pytest.mark.parametrize('name', list(VARIANTS))
def test_eager_and_graph_replayed_frames_stay_bitwise_equal(monkeypatch, name):
    v = VARIANTS[name]
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)
        m = make_model(**v['kw']).cuda()
        outs.append(rollout(m, v, 4, B, 3))
        if rows == '4096':                                 # the hooks are part of the graph key: off after on replays its own graphs
            with hooks(0, 0):
                outs.append(rollout(m, v, 4, B, 3))
            outs.append(rollout(m, v, 4, B, 3))
    for o in outs[1:]:
        same(outs[0], o, 'graph')


def test_below_the_family_rule_nothing_changes(monkeypatch):
    """B = 8: 72 rows, the full projection is no persistent split-operand call and the hooks change neither the launches nor the bits."""
    monkeypatch.setenv('D4_GRAPH_MAX_ROWS', '0')
    v = VARIANTS['tasks']
    m = make_model(**v['kw']).cuda()
    rollout(m, v, 1, 8, 5)
    all_arms(m, v, lambda: rollout(m, v, T, 8, 21), probe=False)
    o = all_arms(m, v, lambda: rollout(m, v, T, 8, 21), probe=False)
    assert len({a['count'] for a in o.values()}) == 1 and o['off']['count'] > 0
    for arm in ('l0', 'ck', 'on'):
        same(o['off']['res'], o[arm]['res'], arm)
