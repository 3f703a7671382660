"""GPU: state that outlives a call.  DynamicsWorldModel and VideoTokenizer keep images of the trunk weights inside their engines (gamma-folded
fused projections, split planes, bf16 mirrors, the register rows projected once, captured frame graphs); Python decides from the module tree,
`data_ptr()` and `Tensor._version` when to rebuild them.  Every test here is writer x reader x arithmetic (tests/coherence_cases.py):

    reader(model)  ->  writer(model)  ->  reader(model)   against   reader(a FRESH instance loaded with model.state_dict())

compared with `torch.equal` on every returned tensor: both instances run the same kernels on the same shapes in one process.  Two controls are
asserted, not assumed: two fresh instances from one state dict agree bit for bit in every arithmetic mode (otherwise bit equality would be the
wrong bar), and the reading after the write differs from the reading before it (otherwise a stale engine and a fresh one could agree by
accident).  No over-invalidation: a call with nothing written before it enqueues exactly the steady-state number of launches."""
import copy
import gc

import pytest
import torch

import coherence_cases as CC
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu


def same(a, b, what):
    bad = CC.differing(a, b)
    assert not bad, f'{what}: {bad} differ' + ''.join(
        f'\n  {k}: max abs diff {(a[k].double() - b[k].double()).abs().max().item():.3e}' for k in bad if a[k].shape == b[k].shape)


def moved(before, after, must, what):
    changed = CC.differing(before, after)
    still = [k for k in must if k not in changed]
    assert not still, f'{what}: the write did not move {still} - the case cannot tell a stale engine from a fresh one'


@pytest.fixture(scope='module')
def experience():
    """an Experience WITHOUT agent embeddings, generated once by a model of its own: data for the learn reader, never changed"""
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    m = CC.dynamics().cuda()
    return m.generate(CC.FRAMES, batch_size=CC.BATCH, return_for_policy_optimization=True, store_agent_embed=False, noise=CC.noise(m, seed=53))


def run_case(build, reader, writer, must, what, **ctx):
    m = build().cuda()
    before = reader(m, **ctx)
    writer(m)
    after = reader(m, **ctx)
    moved(before, after, must, what)
    same(after, reader(CC.fresh_like(m, build), **ctx), what + ': the instance written to against a fresh one')
    again = reader(m, **ctx)
    same(after, again, what + ': a second reading after the write')


# ------------------------------------------------------------------------------------------------------------------- controls
@pytest.mark.parametrize('reader', sorted(CC.READERS))
@pytest.mark.parametrize('mode', CC.MODES)
def test_two_fresh_instances_agree_bit_for_bit(mode, reader, experience):
    build = lambda: CC.dynamics(mode)
    read = CC.READERS[reader][0]
    first = build().cuda()
    a = read(first, experience=experience)
    same(a, read(CC.fresh_like(first, build), experience=experience), f'{mode} {reader}: fresh against fresh')
    same(a, read(first, experience=experience), f'{mode} {reader}: the same instance twice')


@pytest.mark.parametrize('reader', sorted(CC.TOK_READERS))
@pytest.mark.parametrize('mode', CC.TOK_MODES)
def test_two_fresh_tokenizers_agree_bit_for_bit(mode, reader):
    build = lambda: CC.tokenizer(mode)
    first = build().cuda()
    a = CC.TOK_READERS[reader](first)
    same(a, CC.TOK_READERS[reader](CC.fresh_like(first, build)), f'tokenizer {mode} {reader}: fresh against fresh')


# ------------------------------------------------------------------------------------------------------------------- world model
@pytest.mark.parametrize('graph_rows', CC.GRAPH_ROWS)
@pytest.mark.parametrize('writer', sorted(CC.WRITERS))
def test_writer_reaches_generate(writer, graph_rows, monkeypatch):
    monkeypatch.setenv('D4_GRAPH_MAX_ROWS', graph_rows)         # read at engine creation; captured frame graphs bake addresses
    fn, moves = CC.WRITERS[writer]
    read, must = CC.READERS['generate']
    run_case(CC.dynamics, read, fn, must[moves], f'{writer} -> generate (graph rows {graph_rows})')


# (an inference forward returns nothing the heads compute: a writer that moves only the heads has no forward case — it could not be told
# from no write at all)
OTHER_READERS = [(w, r) for w in sorted(CC.WRITERS) for r in ('forward', 'learn') if CC.READERS[r][1][CC.WRITERS[w][1]]]


@pytest.mark.parametrize('writer,reader', OTHER_READERS)
def test_writer_reaches_forward_and_learn(writer, reader, experience):
    fn, moves = CC.WRITERS[writer]
    read, must = CC.READERS[reader]
    run_case(CC.dynamics, read, fn, must[moves], f'{writer} -> {reader}', experience=experience)


MODE_WRITERS = [w for w in sorted(CC.WRITERS) if w.startswith('muon_') or w == 'load_state_dict_assign']


@pytest.mark.parametrize('mode', [m for m in CC.MODES if m != CC.DEFAULT_MODE])
@pytest.mark.parametrize('writer', MODE_WRITERS)
def test_writer_reaches_generate_in_every_arithmetic(writer, mode):
    """each matmul_dtype keeps other derived images: f32 fused projections, bf16x3 / fp16x2 planes, bf16 mirrors"""
    fn, moves = CC.WRITERS[writer]
    read, must = CC.READERS['generate']
    run_case(lambda: CC.dynamics(mode), read, fn, must[moves], f'{writer} -> generate ({mode})')


def test_data_writes_are_stale_until_invalidate_prepared():
    """The documented invisible write: `.data` shows on no counter, `invalidate_prepared()` is the remedy and then the engine is fresh.  The weight
    written is one the engine reads through its prepared image only (the feedforward's output projection, as in
    test_trunk_weight_updates_reach_the_prepared_images): a tensor the kernels also read in place would give a mixture, not the old output."""
    m = CC.dynamics().cuda()
    before = CC.r_generate(m)
    CC.param(m, CC.SCALED[1]).data.mul_(0.5)
    same(before, CC.r_generate(m), 'a .data write is not seen (documented)')
    m.invalidate_prepared()
    after = CC.r_generate(m)
    moved(before, after, CC.READERS['generate'][1]['trunk'], '.data write + invalidate_prepared')
    same(after, CC.r_generate(CC.fresh_like(m, CC.dynamics)), 'after invalidate_prepared, against a fresh instance')


def test_deep_copy_after_generate_is_an_independent_model():
    m = CC.dynamics().cuda()
    a0 = CC.r_generate(m)
    twin = copy.deepcopy(m)
    assert twin._engine is None and twin._ws is None and twin._groups == {}
    b0 = CC.r_generate(twin)
    same(a0, b0, 'the copy against its original')
    assert twin._engine is not None and twin._engine.value != m._engine.value
    with torch.no_grad():
        CC.param(twin, CC.SCALED[1]).mul_(0.5)
    b1 = CC.r_generate(twin)
    moved(b0, b1, CC.READERS['generate'][1]['trunk'], 'scaling a trunk weight of the copy')
    same(a0, CC.r_generate(m), 'the original after a write to the copy')
    same(b1, CC.r_generate(CC.fresh_like(twin, CC.dynamics)), 'the copy written to against a fresh instance')
    del twin, b0, b1
    gc.collect()
    same(a0, CC.r_generate(m), 'the original after the copy was deleted')


# ------------------------------------------------------------------------------------------------------------------- no over-invalidation
def launches(fn):
    lib = _lib.load()
    lib.d4_debug_switch(b'launch_count', 0)
    fn()
    return lib.d4_debug_switch(b'launch_count', 0)


@pytest.mark.parametrize('graph_rows', CC.GRAPH_ROWS)
def test_generate_re_prepares_only_after_a_write(graph_rows, monkeypatch):
    """A fix that re-prepared on every call would pass every test above.  d4_engine_prepare launches eagerly, so the counter sees it."""
    monkeypatch.setenv('D4_GRAPH_MAX_ROWS', graph_rows)
    m = CC.dynamics().cuda()
    call = lambda: CC.r_generate(m)
    first, second, third = launches(call), launches(call), launches(call)
    print(f'generate (graph rows {graph_rows}): launches {first}, {second}, {third}')
    assert third == second <= first
    CC.w_mul(m)
    after_write = launches(call)
    assert after_write > second, (after_write, second)
    assert launches(call) == second
    CC.w_muon(m, 'fp32_clip')
    assert launches(call) > second
    assert launches(call) == second


@pytest.mark.parametrize('graph_rows', CC.GRAPH_ROWS)
def test_a_step_of_the_heads_alone_re_prepares_nothing(graph_rows, monkeypatch):
    """The flagship loop (DreamTrainer: generate, learn, native AdamW on the two flat head groups) marks the head parameters as mutated, and the
    engine keeps no image of them: the next generate enqueues the steady-state number of launches.  The first step is a warm-up — the learner's
    workspace makes the engine grow once, which rightly prepares everything again."""
    from dreamer4_amd import DreamTrainer
    monkeypatch.setenv('D4_GRAPH_MAX_ROWS', graph_rows)
    m = CC.dynamics().cuda()
    # (the reference's learning rate: at 1e-2 the first step already saturates this small policy, and a log-probability of exactly 0 moves no more)
    trainer = DreamTrainer(m, batch_size=CC.BATCH, generate_timesteps=CC.FRAMES - 1, learning_rate=3e-4, seed=5)
    trainer.train_step()
    call = lambda: CC.r_generate(m)
    first, second, third = launches(call), launches(call), launches(call)
    assert third == second <= first
    before = call()
    versions = [p._version for p in m.value_head_parameters()]
    trainer.train_step()
    assert all(p._version > v for p, v in zip(m.value_head_parameters(), versions)), 'the native head step is a visible writer'
    assert launches(call) == second
    moved(before, call(), CC.READERS['generate'][1]['heads'], 'a DreamTrainer step')


@pytest.mark.parametrize('mode', CC.TOK_MODES)
def test_decode_re_prepares_only_after_a_write(mode):
    tok = CC.tokenizer(mode).cuda()
    call = lambda: CC.r_decode(tok)
    first, second, third = launches(call), launches(call), launches(call)
    print(f'decode ({mode}): launches {first}, {second}, {third}')
    assert third == second <= first
    CC.tw_mul(tok)
    assert launches(call) > second
    assert launches(call) == second
    CC.tw_muon(tok)
    assert launches(call) > second
    assert launches(call) == second


# ------------------------------------------------------------------------------------------------------------------- tokenizer
@pytest.mark.parametrize('mode', CC.TOK_MODES)
@pytest.mark.parametrize('reader', sorted(CC.TOK_READERS))
@pytest.mark.parametrize('writer', sorted(CC.TOK_WRITERS))
def test_tokenizer_writer_reaches_reader(writer, reader, mode):
    run_case(lambda: CC.tokenizer(mode), CC.TOK_READERS[reader], CC.TOK_WRITERS[writer], ('latents',) if reader == 'tokenize' else ('video',),
             f'tokenizer {writer} -> {reader} ({mode})')


def nested(tok=None):
    return CC.dynamics(video_tokenizer=CC.tokenizer() if tok is None else tok, copy_video_tokenizer=False)


def r_prompted(m, **_):
    tok = m.video_tokenizer
    x = CC.tok_inputs(tok)
    nz = dict(CC.noise(m), video=x['noise'])
    e = m.generate(CC.FRAMES, batch_size=CC.BATCH, prompt=x['video'][:, :, :1], return_rewards_per_frame=True, return_agent_actions=True,
                   return_log_probs_and_values=True, noise=nz)
    return dict(prompt_latents=e.latents[:, :1], latents=e.latents, video=e.video, values=e.values, actions=e.actions.discrete)


def test_muon_steps_of_a_nested_tokenizer_reach_a_prompted_generate():
    """DynamicsWorldModel(video_tokenizer=tok, copy_video_tokenizer=False): the tokenizer's parameters are the caller's, stepped by Muon, read through
    generate(prompt=video), which tokenizes the prompt (encoder engine) and decodes the rollout (decoder engine)."""
    same(r_prompted(nested().cuda()), r_prompted(nested().cuda()), 'control: two fresh nested models')
    run_case(nested, r_prompted, lambda m: CC.tw_muon(m.video_tokenizer), ('prompt_latents', 'latents', 'video'), 'muon on the nested tokenizer -> generate(prompt=)')
