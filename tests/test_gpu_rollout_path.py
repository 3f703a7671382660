"""GPU: what the rollout keeps on its per-frame path.

Two changes of d4_rollout, each behind a d4_debug_switch hook that restores the former path:
  rollout_clean_agent_row  the clean evaluation of a frame (the one that feeds the heads) computes no latent prediction and, on the engines
                           that can, runs its final stage on the agent row alone;
  rollout_batched_heads    the value and reward heads run once after the frame loop over all B * F agent rows.
Everything that feeds back into the rollout (actions, log-probs, latents, terminals, lens, agent embedding, time cache) must be bit-identical
with either hook on or off; values and rewards are bit-identical at one new frame per call and differ by fp32 rounding only beyond (another
GEMM configuration runs at B * F rows): they are checked against oracle/restate.py with the tolerance of tests/test_gpu_generate.py.

Three shapes: a tiny model on the separate kernels (dim 64, 2 heads of 32, depth 2 with a time layer, 3 frames after a 1-frame prompt), the
default architecture at dim 512 / depth 2 with 192 trajectories (the per-frame fused kernels write the agent-only compaction), and B = 1, F = 1."""
import pytest
import torch

from dreamer4_amd import _lib
from oracle import restate
from util import make_noise, oracle_config, oracle_weights, randomize_weights, small_model

pytestmark = pytest.mark.gpu
ATOL, RTOL = 2e-4, 1e-4          # tests/test_gpu_generate.py
HOOK_A, HOOK_B = b'rollout_clean_agent_row', b'rollout_batched_heads'


def tiny_model():
    return small_model(dim=64, depth=2, time_block_every=2, attn_heads=2, attn_dim_head=32, num_latent_tokens=4)


def wide_model(**kw):
    from dreamer4_amd import DynamicsWorldModel
    torch.manual_seed(0)
    return randomize_weights(DynamicsWorldModel(dim=512, dim_latent=32, num_latent_tokens=32, depth=2, num_discrete_actions=4, **kw), terminal_bias=-10.)


SHAPES = {
    # name: (model, batch, time_steps, prompt frames)
    'tiny_prompt': (tiny_model, 3, 4, 1),
    'dim512_b192': (wide_model, 192, 2, 0),
    'b1_f1': (tiny_model, 1, 1, 0),
}


class hooks:
    def __init__(self, a, b):
        self.want = ((HOOK_A, a), (HOOK_B, b))

    def __enter__(self):
        lib = _lib.load()
        self.old = [(n, lib.d4_debug_switch(n, v)) for n, v in self.want]
        assert all(o in (0, 1) for _, o in self.old)

    def __exit__(self, *exc):
        lib = _lib.load()
        for n, o in self.old:
            lib.d4_debug_switch(n, o)


def kv_of(m, tc):
    """the time KV cache a rollout leaves behind (empty for a trunk without time layers)"""
    return tc.kv().clone() if m.depth // m.time_block_every > 0 else torch.empty(0)


def rollout(m, T, B, nz, prompt, a, b):
    with hooks(a, b):
        e, tc = m.generate(T, batch_size=B, return_for_policy_optimization=True, return_time_cache=True, noise=nz, **prompt)
        return e, kv_of(m, tc)


def fields(e):
    """every tensor generate returns, by name"""
    out = dict(latents=e.latents, agent_embed=e.agent_embed, rewards=e.rewards, values=e.values, log_probs=e.log_probs.discrete,
               unembeds=e.old_action_unembeds.discrete, actions=e.actions.discrete, lens=e.lens, terminals=e.terminals,
               is_truncated=e.is_truncated, episode_return=e.episode_return)
    assert all(torch.is_tensor(v) for v in out.values())
    return out


ROUNDED = ('values', 'rewards', 'episode_return')         # what the batched heads may round differently at F > 1


@pytest.fixture(scope='module', params=list(SHAPES))
def runs(request):
    """One model per shape; the oracle once; the rollout on the former path (both hooks off), with each hook alone and with both (the default)."""
    assert torch.cuda.is_available()
    make, B, T, P = SHAPES[request.param]
    m = make()
    cfg, W = oracle_config(m), oracle_weights(m)
    nz = make_noise(cfg, T, B, 41)
    prompt = {}
    if P:
        g = torch.Generator().manual_seed(7)
        prompt = dict(prompt_latents=torch.randn(B, P, cfg.num_latent_tokens, cfg.dim_latent, generator=g).clamp(-1, 1),
                      prompt_discrete_actions=torch.randint(0, cfg.num_discrete_actions[0], (B, P, 1), generator=g),
                      prompt_rewards=torch.zeros(B, P))
    ref = restate.generate(cfg, W, T, batch_size=B, noise=nz, **prompt)
    m = m.cuda()
    out = {(a, b): rollout(m, T, B, nz, prompt, a, b) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))}
    return dict(name=request.param, m=m, cfg=cfg, nz=nz, ref=ref, F=T - P, out=out)


def test_hooks_exist_and_default_on():
    lib = _lib.load()
    for n in (HOOK_A, HOOK_B):
        assert lib.d4_debug_switch(n, 1) == 1


def test_clean_evaluation_without_prediction_is_bitwise_the_former_path(runs):
    """Hook A on vs off (B off): every tensor generate returns and the time cache, bit for bit."""
    (e0, kv0), (e1, kv1) = runs['out'][(0, 0)], runs['out'][(1, 0)]
    f0, f1 = fields(e0), fields(e1)
    for k in f0:
        assert torch.equal(f0[k], f1[k]), k
    assert torch.equal(kv0, kv1)


@pytest.mark.parametrize('a', [0, 1])
def test_batched_heads_leave_the_rollout_bitwise_and_round_only_values_and_rewards(runs, a):
    """Hook B on vs off: what feeds back into the rollout is bit-identical for every F; at F = 1 values and rewards too; at F > 1 they differ by
    no more than the tolerance they are held to against the oracle."""
    (e0, kv0), (e1, kv1) = runs['out'][(a, 0)], runs['out'][(a, 1)]
    f0, f1 = fields(e0), fields(e1)
    for k in f0:
        if k in ROUNDED and runs['F'] > 1:
            d = (f0[k] - f1[k]).abs().max().item()
            print(f"{runs['name']} hook A {a}: {k} on/off max abs diff {d:.3e}")
            assert torch.allclose(f1[k], f0[k], atol=ATOL, rtol=RTOL), (k, d)
        else:
            assert torch.equal(f0[k], f1[k]), k
    assert torch.equal(kv0, kv1)


def well_posed(ref, nz, cfg, margin=1e-3):
    """trajectories whose sampled actions are decided by a top-2 margin of (logit + Gumbel) above fp32 noise (util.rollout_parity's rule)"""
    lg = ref['old_action_unembeds']
    B, Fa = lg.shape[:2]
    u = nz['gumbel_u'][:Fa].transpose(0, 1)[:B]
    z = lg - torch.log((-torch.log(u.clamp(min=1e-20))).clamp(min=1e-20))
    well, o = torch.ones(B, dtype=torch.bool), 0
    for n in cfg.num_discrete_actions:
        top = z[..., o:o + n].topk(2, dim=-1).values
        well &= ((top[..., 0] - top[..., 1]).min(dim=1).values >= margin)
        o += n
    return well


def test_values_and_rewards_vs_oracle(runs):
    """Both changes on (the default): values and rewards against oracle/restate.py with test_gpu_generate's tolerance, integers exact — on the
    trajectories whose action choices are well posed (all of them at the small batches)."""
    e, _ = runs['out'][(1, 1)]
    ref, F_ = runs['ref'], runs['F']
    assert e.latents.shape[1] == ref['latents'].shape[1]
    well = well_posed(ref, runs['nz'], runs['cfg'])
    assert well.any()
    acts = e.actions.discrete.cpu()
    assert torch.equal(acts[well], ref['actions'][well])
    for name, got, want in (('values', e.values, ref['values']), ('rewards', e.rewards, ref['rewards']), ('agent_embed', e.agent_embed, ref['agent_embed']),
                            ('latents', e.latents, ref['latents'])):
        got, want = got.cpu().float()[well], want.float()[well]
        d = (got - want).abs().max().item()
        print(f"{runs['name']}: {name} vs oracle max abs diff {d:.3e} over {int(well.sum())} trajectories, {F_} frames")
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), (name, d)


def test_wm_forward_after_a_rollout_still_returns_the_prediction(runs):
    """d4_wm_forward on the engine that just ran a rollout without predictions: prediction and agent embedding bit-identical to a fresh engine's
    (nothing of the need_pred = false state outlives the evaluation)."""
    m, cfg = runs['m'], runs['cfg']
    make, B, T, P = SHAPES[runs['name']]
    B, T = min(B, 4), 1                                        # (one frame: the engine the rollout used is large enough, so it is the one that runs)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(B, T, cfg.num_latent_tokens, cfg.dim_latent, generator=g)
    sig = torch.randint(0, cfg.max_steps, (B, T), generator=g)
    nz = make_noise(cfg, 2, B, 5)
    m.generate(2, batch_size=B, return_for_policy_optimization=True, noise=nz)          # leaves the engine after a clean evaluation without prediction
    pred, (agent, _) = m(latents=lat, signal_levels=sig, step_sizes=4)
    fresh = make().cuda()
    pred0, (agent0, _) = fresh(latents=lat, signal_levels=sig, step_sizes=4)
    assert torch.equal(pred, pred0) and torch.equal(agent, agent0)
    assert pred.abs().max().item() > 0


@pytest.mark.parametrize('make,B', [(tiny_model, 1), (tiny_model, 3), (wide_model, 2)])
def test_one_frame_calls_make_the_same_launches_and_bits(make, B, monkeypatch):
    """F = 1 (the env-step pattern, chained): with the batched heads the call enqueues exactly as many kernels as the per-frame path and returns the
    same bits, values and rewards included.  Frames are enqueued eagerly here so that the host-side launch counter sees every kernel."""
    monkeypatch.setenv('D4_GRAPH_MAX_ROWS', '0')               # read at engine creation
    lib = _lib.load()
    m = make().cuda()
    cfg = oracle_config(m)
    nz = make_noise(cfg, 3, B, 9)
    m.generate(1, batch_size=B, return_for_policy_optimization=True, noise={k: v[:1] for k, v in nz.items()})      # (weight preparation is not part of a call)
    res = {}
    for b in (0, 1):
        with hooks(1, b):
            tc, lat, act, outs, counts = None, None, None, [], []
            for i in range(3):
                kw = dict(prompt_latents=lat, prompt_discrete_actions=act) if i > 0 else {}
                lib.d4_debug_switch(b'launch_count', 0)
                e, tc = m.generate(i + 1, batch_size=B, return_for_policy_optimization=True, time_cache=tc, return_time_cache=True,
                                   noise={k: v[i:i + 1] for k, v in nz.items()}, **kw)
                counts.append(lib.d4_debug_switch(b'launch_count', 0))
                lat, act = e.latents, e.actions.discrete
                outs.append(fields(e))
            res[b] = (outs, counts, kv_of(m, tc))
    (o0, c0, kv0), (o1, c1, kv1) = res[0], res[1]
    print(f'launches per one-frame call: per-frame heads {c0}, batched heads {c1}')
    assert c0 == c1 and min(c0) > 0
    for f0, f1 in zip(o0, o1):
        for k in f0:
            assert torch.equal(f0[k], f1[k]), k
    assert torch.equal(kv0, kv1)


@pytest.mark.parametrize('make,B,T', [(tiny_model, 3, 5), (wide_model, 4, 4)])
def test_eager_and_graph_replayed_frames_stay_bitwise_equal(make, B, T, monkeypatch):
    """Both changes on: the same rollout enqueued eagerly and replayed from hipGraphs (the clean evaluation without its prediction is what the
    graph captures) is bit-identical — the pattern of test_gpu_generate's eager / replay test."""
    outs = []
    for rows in ('0', '4096'):
        monkeypatch.setenv('D4_GRAPH_MAX_ROWS', rows)
        m = make().cuda()
        nz = make_noise(oracle_config(m), T, B, 3)
        e, tc = m.generate(T, batch_size=B, return_for_policy_optimization=True, return_time_cache=True, noise=nz)
        outs.append((fields(e), kv_of(m, tc)))
    (a, ka), (b, kb) = outs
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ka, kb)


def test_engine_history_serves_a_caller_without_agent_embed(monkeypatch):
    """A caller of d4_rollout that passes no agent_embed output: the batched heads read the engine's own [B][F][D] history and return the values
    and rewards of the call that passes one, bit for bit (the same rows through the same launches)."""
    lib = _lib.load()
    m = tiny_model().cuda()
    nz = make_noise(oracle_config(m), 4, 3, 13)
    want = fields(m.generate(4, batch_size=3, return_for_policy_optimization=True, noise=nz))
    real = lib.d4_rollout

    def without_agent_embed(engine, io_ref, stream):
        io_ref._obj.agent_embed = None
        return real(engine, io_ref, stream)

    monkeypatch.setattr(lib, 'd4_rollout', without_agent_embed)
    got = fields(m.generate(4, batch_size=3, return_for_policy_optimization=True, noise=nz))
    for k in want:
        if k != 'agent_embed':                                     # (not written by this call)
            assert torch.equal(want[k], got[k]), k
