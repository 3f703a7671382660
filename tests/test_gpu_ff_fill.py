"""GPU: the pools' old keys ride in the preceding feedforward's input projection.

The persistent split-operand kernel walks a launch in rounds of one 128 x 128 tile per CU; its last partial round leaves workgroups idle.  The filled form
(gemm_x3sk_fill_kernel) runs 128 x 64 tiles of an independent f32-input product (the LDS-DMA family's 8-wave configuration) on them.  The engine hands it
the first rows of the next pool's key problem (d4_debug_switch "ff_fill_pool_keys": default 1, 0 = the plain launches); the pool's own key problem then
starts behind those rows.  Every output keeps its bits.

Operator tests: d4_gemm_run_fill against the two plain launches (d4_gemm_run: the persistent kernel, one configuration of the LDS-DMA family), torch.equal
on both outputs inside a NaN guard pattern; partial tile counts write the family's first tiles and nothing else; the launcher's refusals.

Engine tests (dim 512: the SiLU-GLU input projection is 2752 columns = 22 tile columns; B = 128 frames of 14 / 15 rows = 14 / 15 tile rows: 308 / 330 tiles,
one whole round on 256 CUs and a partial one; depth 3: two in-loop pools): hook on against hook off, torch.equal on every output, equal launch counts."""
import ctypes as C
import os

import pytest
import torch

from dreamer4_amd import _lib
from util import make_noise, oracle_config, randomize_weights

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOK = b'ff_fill_pool_keys'
RMS, SWIGLU = _lib.GEMM_RMS_ROWSCALE, _lib.GEMM_SWIGLU
EPS = 1.1920928955078125e-07
GUARD = 0x7FC12345                                          # a NaN bit pattern no kernel produces
PAD = 3                                                     # guard rows on either side of an output
V2_128x64_8, V2_64x64 = 2, 0                                # configurations of the LDS-DMA family (csrc/gemm2.hip)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def guard(rows, cols):
    return torch.full((rows + 2 * PAD, cols), GUARD, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.view(torch.int32)


def pads_intact(t):
    return bool((bits(t[:PAD]) == GUARD).all() and (bits(t[-PAD:]) == GUARD).all())


def desc(**f):
    d = _lib.GemmDesc()
    base = dict(rms_eps=EPS, batch=1, c2_last=1)
    base.update(f)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_capacity(M, N):
    P = cus()
    T = -(-M // 128) * -(-N // 128)
    return P - T % P if T // P >= 1 and T % P else 0


class Main:
    """A call of the persistent split-operand kernel: operands, its plain launch and the descriptor of a launch into a fresh guarded output."""

    def __init__(self, lib, M, N, K, flags, bias, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.M, self.N, self.K, self.flags = M, N, K, flags
        self.A = torch.randn(M, K, device=DEV, generator=g)
        self.A[1] = 0.                                      # an all-zero row: the eps path of the row scale
        W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
        self.bias = torch.randn(N, device=DEV, generator=g) if bias else None
        n = W.numel()
        self.plane = (n + 7) // 8 * 8
        self.W3 = torch.zeros(3 * self.plane, dtype=torch.bfloat16, device=DEV)
        _lib.check(lib.d4_split_bf16x3(_lib.ptr(W), _lib.ptr(self.W3), n, self.plane, stream()))
        self.cols = N // 2 if flags & SWIGLU else N
        self.plain = self.out()
        _lib.check(lib.d4_gemm_run(C.byref(self.desc(self.plain)), _lib.GEMM_X3SK, 0, stream()))
        torch.cuda.synchronize()
        assert pads_intact(self.plain) and not torch.isnan(self.plain[PAD:-PAD]).any()

    def out(self):
        return guard(self.M, self.cols)

    def desc(self, out, **kw):
        f = dict(A=dptr(self.A), lda=self.K, W=self.W3.data_ptr(), ldw=self.K, C=dptr(out, PAD * self.cols), ldc=self.cols, bias=dptr(self.bias), M=self.M, N=self.N,
                 K=self.K, flags=self.flags, Wb=self.W3.data_ptr(), wplane=self.plane)
        f.update(kw)
        return desc(**f)


class Fill:
    """An f32-input product: operands, its plain launch on one configuration of the LDS-DMA family."""

    def __init__(self, lib, M, N, K, rms, bias, seed, cfg=V2_128x64_8):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.M, self.N, self.K, self.flags = M, N, K, RMS if rms else 0
        self.A = torch.randn(M, K, device=DEV, generator=g)
        self.A[M // 2] = 0.
        self.W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
        self.bias = torch.randn(N, device=DEV, generator=g) if bias else None
        self.plain = self.out()
        _lib.check(lib.d4_gemm_run(C.byref(self.desc(self.plain)), _lib.GEMM_V2, cfg, stream()))
        torch.cuda.synchronize()
        assert pads_intact(self.plain) and not torch.isnan(self.plain[PAD:-PAD]).any()

    @property
    def tiles(self):
        return -(-self.M // 128) * -(-self.N // 64)

    def out(self):
        return guard(self.M, self.N)

    def desc(self, out, **kw):
        f = dict(A=dptr(self.A), lda=self.K, W=dptr(self.W), ldw=self.K, C=dptr(out, PAD * self.N), ldc=self.N, bias=dptr(self.bias), M=self.M, N=self.N, K=self.K,
                 flags=self.flags)
        f.update(kw)
        return desc(**f)

    def first_tiles(self, count):
        """mask [M][N] of the first `count` 128 x 64 tiles in the family's block order (csrc/gemm2_body.h: eight bands, one per XCD)"""
        nbm, nbn = -(-self.M // 128), -(-self.N // 64)
        nblk, nx = nbm * nbn, 8
        q, r = divmod(nblk, nx)
        mask = torch.zeros(self.M, self.N, dtype=torch.bool, device=DEV)
        for t in range(count):
            x, o = t % nx, t // nx
            bid = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + o
            bm, bn = divmod(bid, nbn)
            mask[bm * 128:(bm + 1) * 128, bn * 64:(bn + 1) * 64] = True
        return mask


@pytest.fixture(scope='module')
def mains(lib):
    return {'plain': Main(lib, 2176, 2048, 512, 0, False, 1),                 # 272 tiles: 240 idle workgroups on 256 CUs
            'swiglu': Main(lib, 1792, 2752, 512, RMS | SWIGLU, True, 2),      # 308 tiles; the feedforward's input projection at dim 512 (2 x 1376 packed
                                                                              # columns: the SiLU-GLU epilogue needs N % 64 == 0, so not 2 x 1368 = 2736)
            'bias': Main(lib, 2176, 2048, 64, 0, True, 3)}                    # bias, no row scale; two k-tiles


# (main, rows, N, K, row scale, bias, configuration of the plain launch)
FILLS = (('plain', 128, 256, 512, True, False, V2_128x64_8),
         ('plain', 4864, 256, 512, True, False, V2_64x64),
         ('plain', 4864 - 37, 192, 512, False, True, V2_128x64_8),
         ('swiglu', 4864, 256, 512, True, False, V2_128x64_8),
         ('swiglu', 4864 - 37, 256, 64, True, True, V2_64x64),
         ('swiglu', 128, 192, 64, False, False, V2_128x64_8),
         ('bias', 4864 - 37, 192, 512, True, False, V2_128x64_8),
         ('bias', 4864, 256, 64, False, False, V2_128x64_8))


def test_capacity_is_the_idle_workgroups_of_the_last_round(lib, mains):
    for m in mains.values():
        cap = lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain)))
        assert cap == expected_capacity(m.M, m.N) and cap > 0, (m.M, m.N, cap)
    m = mains['plain']
    assert lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain, M=1024))) == 0            # 128 tiles: less than one whole round
    assert lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain, M=2048))) == 0            # 256 tiles: no partial round
    assert lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain, batch=2))) == 0


@pytest.mark.parametrize('case', FILLS, ids=lambda c: '-'.join(map(str, c)))
def test_filled_launch_is_the_two_plain_launches(lib, mains, case):
    name, rows, N, K, rms, bias, cfg = case
    m = mains[name]
    f = Fill(lib, rows, N, K, rms, bias, seed=rows + N + K, cfg=cfg)
    assert f.tiles <= lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain)))
    mo, fo = m.out(), f.out()
    _lib.check(lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(f.desc(fo)), f.tiles, stream()))
    torch.cuda.synchronize()
    assert torch.equal(mo[PAD:-PAD], m.plain[PAD:-PAD]) and pads_intact(mo)
    assert torch.equal(fo[PAD:-PAD], f.plain[PAD:-PAD]) and pads_intact(fo)


@pytest.mark.parametrize('name', ['plain', 'swiglu'])
def test_partial_tile_counts_write_the_first_tiles_only(lib, mains, name):
    m = mains[name]
    cap = lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain)))
    f = Fill(lib, 128 * -(-cap // 4) - 37, 256, 512, True, False, seed=cap)           # at least `cap` tiles; a partly filled last row block
    assert f.tiles >= cap
    for count in (0, 1, cap - 1, cap):
        mo, fo = m.out(), f.out()
        _lib.check(lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(f.desc(fo)), count, stream()))
        torch.cuda.synchronize()
        assert torch.equal(mo[PAD:-PAD], m.plain[PAD:-PAD]) and pads_intact(mo), count
        mask = f.first_tiles(count)
        assert int(mask.any(dim=1).sum()) > 0 or count == 0
        want = torch.where(mask, bits(f.plain[PAD:-PAD]), torch.full_like(bits(f.plain[PAD:-PAD]), GUARD))
        assert torch.equal(bits(fo[PAD:-PAD]), want) and pads_intact(fo), count
    # no fill descriptor at all with no tiles
    mo = m.out()
    _lib.check(lib.d4_gemm_run_fill(C.byref(m.desc(mo)), None, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(mo[PAD:-PAD], m.plain[PAD:-PAD]) and pads_intact(mo)


def test_refusals_launch_nothing(lib, mains):
    m = mains['plain']
    cap = lib.d4_gemm_fill_capacity(C.byref(m.desc(m.plain)))
    big = Fill(lib, 128 * (cap // 4 + 1), 256, 64, True, False, seed=5)
    small = Fill(lib, 256, 256, 64, True, False, seed=6)

    def refused(call, word, *outs):
        rc = call()
        torch.cuda.synchronize()
        msg = lib.d4_last_error().decode()
        return rc != 0 and word in msg and all(bool((bits(o) == GUARD).all()) for o in outs)

    mo, fo = m.out(), big.out()
    assert big.tiles >= cap + 1
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(big.desc(fo)), cap + 1, stream()), 'capacity', mo, fo)
    fo = small.out()
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(small.desc(fo)), small.tiles + 1, stream()), 'fill tiles', mo, fo)
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(small.desc(fo, batch=2, M=128, strideA=128 * 64, strideC=128 * 256)), 4, stream()),
                   'fill problem not supported', mo, fo)
    assert refused(lambda: lib.d4_gemm_run_fill_rowmap(C.byref(m.desc(mo)), C.byref(small.desc(fo, M=128)), 4, 4, 8, 2, 4, stream()), 'fill problem not supported', mo, fo)
    res = torch.zeros(256, 256, device=DEV)
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(small.desc(fo, R=dptr(res), ldr=256)), small.tiles, stream()), 'fill problem not supported', mo, fo)
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo)), C.byref(small.desc(fo, flags=_lib.GEMM_SILU)), small.tiles, stream()), 'fill problem not supported', mo, fo)
    # main calls: below one whole round; one the plain launcher refuses (a batch)
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo, M=1024)), C.byref(small.desc(fo)), small.tiles, stream()), 'no whole round', mo, fo)
    assert refused(lambda: lib.d4_gemm_run_fill(C.byref(m.desc(mo, batch=2)), C.byref(small.desc(fo)), small.tiles, stream()), 'main call not supported', mo, fo)


# ------------------------------------------------------------------------------------------------------------------ engine
class hook:
    def __init__(self, value, **others):
        self.want = [(HOOK, value)] + [(k.encode(), v) for k, v in others.items()]

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
    return randomize_weights(DynamicsWorldModel(dim=512, dim_latent=16, num_latent_tokens=8, depth=3, attn_heads=8, attn_dim_head=64, **kw), terminal_bias=-10.)


# 14 rows per frame in a denoise evaluation, 15 in the clean one (the agent row), either way
VARIANTS = {'time': dict(kw=dict(num_discrete_actions=4, time_block_every=2, num_spatial_tokens=4, num_register_tokens=8), act=True),      # space, time, space
            'noaction': dict(kw=dict(time_block_every=3, num_spatial_tokens=4, num_register_tokens=9), act=False)}
B, T = 128, 3
LAYERS = 2                                                  # in-loop pools of a depth-3 trunk: the feedforwards that carry keys


def rollout(m, v, frames, batch, seed, **kw):
    nz = make_noise(oracle_config(m), frames, batch, seed)
    if not v['act']:
        nz = dict(latent=nz['latent'], context=nz['context'], bern_u=nz['bern_u'])
        lat, tc = m.generate(frames, batch_size=batch, return_time_cache=True, noise=nz, **kw)
        out = dict(latents=lat)
    else:
        e, tc = m.generate(frames, batch_size=batch, return_for_policy_optimization=True, return_time_cache=True, noise=nz, **kw)
        out = dict(latents=e.latents, agent_embed=e.agent_embed, rewards=e.rewards, values=e.values, log_probs=e.log_probs.discrete,
                   unembeds=e.old_action_unembeds.discrete, actions=e.actions.discrete, lens=e.lens, terminals=e.terminals, episode_return=e.episode_return)
    out['kv'] = tc.kv().clone() if m.depth // m.time_block_every > 0 else torch.empty(0)
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in out.items()}


def forward(m, batch, frames, seed):
    cfg = oracle_config(m)
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(batch, frames, cfg.num_latent_tokens, cfg.dim_latent, generator=g)
    sig = torch.randint(0, cfg.max_steps, (batch, frames), generator=g)
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4)
    torch.cuda.synchronize()
    return dict(pred=pred.clone(), agent=agent.clone())


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)
    assert a[next(iter(a))].abs().max().item() > 0


def both_arms(run, **others):
    """run() with the hook off and on -> {arm: (outputs, launches, filled launches)}"""
    lib = _lib.load()
    out = {}
    for arm, value in (('off', 0), ('on', 1)):
        with hook(value, **others):
            lib.d4_debug_switch(b'launch_count', 0)
            lib.d4_debug_switch(b'ff_fill_launches', 0)
            res = run()
            out[arm] = (res, lib.d4_debug_switch(b'launch_count', 0), lib.d4_debug_switch(b'ff_fill_launches', 0))
    return out


class eager_engines:
    """D4_GRAPH_MAX_ROWS = 0 while active: it is read whenever an engine is created (a call with more parallel frames creates a new one), and only kernels
    that are enqueued — not replayed from a captured graph — reach the launch counters"""

    def __enter__(self):
        self.old = os.environ.get('D4_GRAPH_MAX_ROWS')
        os.environ['D4_GRAPH_MAX_ROWS'] = '0'

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['D4_GRAPH_MAX_ROWS']
        else:
            os.environ['D4_GRAPH_MAX_ROWS'] = self.old


@pytest.fixture(scope='module', params=list(VARIANTS))
def eager(request):
    v = VARIANTS[request.param]
    with eager_engines():
        m = make_model(**v['kw']).cuda()
        rollout(m, v, 1, B, 5)
        both_arms(lambda: rollout(m, v, T, B, 41))          # each arm meets its GEMM shapes
        yield dict(name=request.param, v=v, m=m, rollout=both_arms(lambda: rollout(m, v, T, B, 41)))


def test_hook_exists_and_defaults_on(lib):
    assert lib.d4_debug_switch(HOOK, 1) == 1


def test_rollout_is_bitwise_and_launch_counts_are_equal(eager):
    off, on = eager['rollout']['off'], eager['rollout']['on']
    print(eager['name'], off[1:], on[1:])
    same(off[0], on[0], 'rollout')
    assert on[1] == off[1] > 0
    assert off[2] == 0 and on[2] == T * 5 * LAYERS          # 4 denoise evaluations + the clean one per frame, every in-loop pool's feedforward


def test_without_the_constant_keys(eager):
    """pool_const_keys off: the key problem starts at slab 0 and so does the fill"""
    m, v = eager['m'], eager['v']
    both_arms(lambda: rollout(m, v, T, B, 41), pool_const_keys=0)
    o = both_arms(lambda: rollout(m, v, T, B, 41), pool_const_keys=0)
    same(o['off'][0], o['on'][0], 'no constant keys')
    same(o['on'][0], eager['rollout']['off'][0], 'against the default')
    assert o['on'][1] == o['off'][1] and o['off'][2] == 0 and o['on'][2] == T * 5 * LAYERS


def test_prompt_pass_then_cached_decode_and_wm_forward(eager):
    m, v = eager['m'], eager['v']
    cfg = oracle_config(m)
    pl = torch.randn(B, 2, cfg.num_latent_tokens, cfg.dim_latent, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    kw = dict(prompt_latents=pl)
    if v['act']:
        kw['prompt_discrete_actions'] = torch.randint(0, 4, (B, 2), generator=torch.Generator().manual_seed(3))
    both_arms(lambda: rollout(m, v, 4, B, 11, **kw))
    o = both_arms(lambda: rollout(m, v, 4, B, 11, **kw))
    same(o['off'][0], o['on'][0], 'prompt')
    assert o['on'][1] == o['off'][1] and o['off'][2] == 0 and o['on'][2] > 0
    both_arms(lambda: forward(m, B, 1, 1))
    o = both_arms(lambda: forward(m, B, 1, 7))
    same(o['off'][0], o['on'][0], 'wm_forward')
    assert o['on'][1] == o['off'][1] and o['off'][2] == 0 and o['on'][2] == LAYERS
    same(rollout(m, v, T, B, 41), eager['rollout']['off'][0], 'rollout after the other calls')


@pytest.mark.parametrize('name', list(VARIANTS))
def test_eager_and_graph_replayed_frames_stay_bitwise_equal(monkeypatch, name):
    v = VARIANTS[name]
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)
        m = make_model(**v['kw']).cuda()
        outs.append(rollout(m, v, T, B, 3))
        if rows == '4096':                                 # the hook is part of the graph key: off after on replays its own graphs
            with hook(0):
                outs.append(rollout(m, v, T, B, 3))
            outs.append(rollout(m, v, T, B, 3))
    for o in outs[1:]:
        same(outs[0], o, 'graph')


def test_below_the_rule_nothing_changes():
    """B = 8: 112 rows, the input projection is no persistent call: same launches, no filled one, same bits."""
    v = VARIANTS['time']
    with eager_engines():
        m = make_model(**v['kw']).cuda()
        rollout(m, v, 1, 8, 5)
        both_arms(lambda: rollout(m, v, T, 8, 21))
        o = both_arms(lambda: rollout(m, v, T, 8, 21))
    assert o['on'][1] == o['off'][1] > 0 and o['on'][2] == 0 and o['off'][2] == 0
    same(o['off'][0], o['on'][0], 'B = 8')
