"""Writers, readers and shapes of the weight-cache coherence tests (tests/test_coherence_host.py, tests/test_gpu_coherence.py).

A WRITER changes a model's parameters the way a user would; a READER runs the model and returns every tensor it produced, by name.  The GPU
tests run reader, writer, reader on one instance and compare the second reading bit for bit with the same reader on a FRESH instance that
carries the first one's state_dict: an engine that went on using images of the old weights cannot pass.  Nothing here touches a device at import."""
import functools

import torch
from torch import nn

import muon_cases as MC
from util import make_noise, oracle_config, small_model

BATCH, FRAMES = 2, 3
MODES = ('fp32', 'fp32_mfma', 'fp32_fp16x2', 'bf16')          # DynamicsWorldModel(matmul_dtype=): each keeps other derived images
DEFAULT_MODE = 'fp32'
GRAPH_ROWS = ('0', '4096')                                   # D4_GRAPH_MAX_ROWS: frames enqueued eagerly / replayed from captured graphs
# trunk tensors a direct write scales: a gamma the fused projection folds in, a weight with split planes / a bf16 mirror, and the rows
# d4_engine_prepare projects once
SCALED = ('transformer.layers.0.2.fn.norm.weight', 'transformer.layers.0.3.fn.proj_out.weight', 'register_tokens')
SWAPPED_TRUNK = 'transformer.layers.2.3.fn.proj_in.weight'
SWAPPED_HEAD = 'value_head.layers.4.1.weight'                # the value head's output Linear
MUON = {'fp32_clip': dict(muon_products='fp32', max_grad_norm=0.5), 'fp32': dict(muon_products='fp32'),
        'bf16_clip': dict(muon_products='bf16', max_grad_norm=0.5), 'bf16': dict(muon_products='bf16')}


def dynamics(mode=DEFAULT_MODE, **over):
    return small_model(matmul_dtype=mode, **over)


def fresh_like(model, build):
    """the reference: a second instance from the same constructor arguments, carrying `model`'s weights by plain copying load_state_dict"""
    ref = build()
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return ref.cuda()


def owner_of(model, key):
    mod = model
    *path, leaf = key.split('.')
    for p in path:
        mod = mod._modules[p]
    return mod, leaf


def param(model, key):
    mod, leaf = owner_of(model, key)
    return mod._parameters[leaf]


# ----------------------------------------------------------------------------------------------------------------------- writers
def set_grads(model, step):
    for k, p in model.named_parameters():
        g = step.get(k)
        p.grad = None if g is None else g.to(p.device)


def w_adamw(m):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    set_grads(m, MC.trajectory_gradients(m)[0])
    opt.step()


def w_sgd(m):
    """(host test: a torch optimiser that needs no device)"""
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    set_grads(m, MC.trajectory_gradients(m)[0])
    opt.step()


def w_mul(m):
    with torch.no_grad():
        for k in SCALED:
            param(m, k).mul_(0.5)


def w_copy(m):
    with torch.no_grad():
        for k in SCALED:
            p = param(m, k)
            p.copy_(p.detach().clone() * 0.5)


def scaled_state_dict(m):
    return {k: (v.detach().clone() * 0.5 if k in SCALED else v.detach().clone()) for k, v in m.state_dict().items()}


def w_load_copying(m):
    m.load_state_dict(scaled_state_dict(m))


def w_load_assign(m):
    m.load_state_dict(scaled_state_dict(m), assign=True)


def w_swap_trunk(m):
    mod, leaf = owner_of(m, SWAPPED_TRUNK)
    setattr(mod, leaf, nn.Parameter(mod._parameters[leaf].detach().clone() * 0.5))


def w_swap_head(m):
    mod, leaf = owner_of(m, SWAPPED_HEAD)
    setattr(mod, leaf, nn.Parameter(mod._parameters[leaf].detach().clone() * 0.5))


def w_muon(m, case='fp32', params=None, muon_params=None):
    """two steps; zero_grad(set_to_none=True) in between, so the second step's gradients are other allocations"""
    from dreamer4_amd import MuonAdamAtan2
    opt = MuonAdamAtan2(m.muon_parameters() if muon_params is None else muon_params, m.parameters() if params is None else params,
                        lr=1e-2, muon_lr=2e-2, **MUON[case])
    steps = MC.trajectory_gradients(m)
    for step in steps[:2]:
        opt.zero_grad(set_to_none=True)
        set_grads(m, step)
        opt.step()
    opt.zero_grad(set_to_none=True)


def w_dream_trainer(m):
    from dreamer4_amd import DreamTrainer
    DreamTrainer(m, batch_size=BATCH, generate_timesteps=FRAMES - 1, learning_rate=1e-2, seed=5).train_step()


def w_cpu_cuda(m):
    """The move itself has to be seen: the scaling in between goes through `.data`, which no version counter notices."""
    m.cpu()
    for k in SCALED:
        param(m, k).data.mul_(0.5)
    m.cuda()


# what each writer moves: 'trunk' (the flow prediction changes, and everything after it), 'heads' (only what the two heads produce changes) or
# 'value_head' (only what the value head produces changes)
WRITERS = {
    'adamw': (w_adamw, 'trunk'), 'mul_': (w_mul, 'trunk'), 'copy_': (w_copy, 'trunk'), 'load_state_dict': (w_load_copying, 'trunk'),
    'load_state_dict_assign': (w_load_assign, 'trunk'), 'swap_trunk_parameter': (w_swap_trunk, 'trunk'),
    'swap_head_parameter': (w_swap_head, 'value_head'), 'dream_trainer_step': (w_dream_trainer, 'heads'), 'cpu_cuda': (w_cpu_cuda, 'trunk'),
    **{f'muon_{case}': (functools.partial(w_muon, case=case), 'trunk') for case in MUON},
}
HOST_WRITERS = {'sgd': w_sgd, 'mul_': w_mul, 'copy_': w_copy, 'load_state_dict': w_load_copying, 'load_state_dict_assign': w_load_assign,
                'swap_trunk_parameter': w_swap_trunk, 'swap_head_parameter': w_swap_head}


# ----------------------------------------------------------------------------------------------------------------------- readers
def noise(m, seed=41):
    return make_noise(oracle_config(m), FRAMES, BATCH, seed)


def r_generate(m, **_):
    e, tc = m.generate(FRAMES, batch_size=BATCH, return_for_policy_optimization=True, return_time_cache=True, noise=noise(m))
    return dict(latents=e.latents, agent_embed=e.agent_embed, rewards=e.rewards, values=e.values, log_probs=e.log_probs.discrete,
                actions=e.actions.discrete, kv=tc.kv())


def forward_inputs(m):
    g = torch.Generator().manual_seed(43)
    n, dl = m.latent_shape
    return dict(latents=torch.randn(BATCH, FRAMES, n, dl, generator=g), signal_levels=torch.randint(0, m.max_steps, (BATCH, FRAMES), generator=g),
                step_sizes=4, discrete_actions=torch.randint(0, m.num_discrete_actions[0], (BATCH, FRAMES, 1), generator=g),
                tasks=torch.randint(0, m.num_tasks, (BATCH,), generator=g))


def r_forward(m, **_):
    pred, (agent, tc) = m(**forward_inputs(m))
    return dict(pred=pred, agent_embed=agent, kv=tc.kv())


def r_learn(m, experience=None, **_):
    """learn_from_experience on an Experience without agent embeddings: the trunk runs again over the stored latents"""
    pl, vl = m.learn_from_experience(experience)
    return dict(policy_loss=pl.detach().clone(), value_loss=vl.detach().clone(),
                policy_grad=m._groups['policy']['grad'].clone(), value_grad=m._groups['value']['grad'].clone())


# reader -> (function, {what a writer moves: the outputs that must then change}); an inference forward returns nothing a head computed
READERS = {'generate': (r_generate, dict(trunk=('latents', 'agent_embed', 'kv', 'values', 'log_probs'), heads=('values', 'log_probs'), value_head=('values',))),
           'forward': (r_forward, dict(trunk=('pred', 'agent_embed', 'kv'), heads=(), value_head=())),
           'learn': (r_learn, dict(trunk=('policy_loss', 'value_loss'), heads=('policy_loss', 'value_loss'), value_head=('value_loss',)))}


def differing(a, b):
    """names of the outputs that are not bit-identical"""
    assert a.keys() == b.keys()
    return [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]


# ----------------------------------------------------------------------------------------------------------------------- tokenizer
TOK_MODES = ('fp32', 'bf16')
TOK_SCALED = ('decoder.transformer.layers.0.3.fn.proj_out.weight', 'encoder_transformer.layers.0.3.fn.proj_out.weight',
              'decoder.transformer.layers.0.2.fn.norm.weight', 'encoder_transformer.layers.0.2.fn.norm.weight')


@functools.lru_cache(maxsize=None)
def tok_fixture():
    import tok_train_cases as TC
    kw, W, _ = TC.fixture()
    return kw, W


def tokenizer(mode='fp32'):
    from dreamer4_amd import VideoTokenizer
    kw, W = tok_fixture()
    tok = VideoTokenizer(**kw, lpips_loss_weight=0., matmul_dtype=mode)
    missing, unexpected = tok.load_state_dict(W, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return tok.eval()


def tok_inputs(tok):
    g = torch.Generator().manual_seed(47)
    video = torch.rand(BATCH, tok.channels, FRAMES, tok.image_height, tok.image_width, generator=g)
    return dict(video=video, latents=torch.rand(BATCH, FRAMES, *tok.latent_shape, generator=g) * 2. - 1., noise=torch.randn(video.shape, generator=g))


def r_tokenize(tok, **_):
    return dict(latents=tok.tokenize(tok_inputs(tok)['video']))


def r_decode(tok, **_):
    x = tok_inputs(tok)
    return dict(video=tok.decode(x['latents'], noise=x['noise']))


def tw_mul(tok):
    with torch.no_grad():
        for k in TOK_SCALED:
            param(tok, k).mul_(0.5)


def tw_load_assign(tok):
    tok.load_state_dict({k: (v.detach().clone() * 0.5 if k in TOK_SCALED else v.detach().clone()) for k, v in tok.state_dict().items()}, assign=True)


def tw_swap(tok):
    for k in TOK_SCALED[:2]:
        mod, leaf = owner_of(tok, k)
        setattr(mod, leaf, nn.Parameter(mod._parameters[leaf].detach().clone() * 0.5))


def tok_gradients(tok):
    g = torch.Generator().manual_seed(13)
    return [{k: torch.randn(p.shape, generator=g) for k, p in tok.named_parameters()} for _ in range(2)]


def tw_muon(tok, case='fp32_clip'):
    from dreamer4_amd import MuonAdamAtan2
    opt = MuonAdamAtan2(tok.muon_parameters(), tok.parameters(), lr=1e-2, muon_lr=2e-2, **MUON[case])
    for step in tok_gradients(tok):
        opt.zero_grad(set_to_none=True)
        set_grads(tok, step)
        opt.step()
    opt.zero_grad(set_to_none=True)


TOK_WRITERS = {'mul_': tw_mul, 'load_state_dict_assign': tw_load_assign, 'swap_parameters': tw_swap,
               'muon_fp32_clip': functools.partial(tw_muon, case='fp32_clip'), 'muon_bf16': functools.partial(tw_muon, case='bf16')}
TOK_READERS = {'tokenize': r_tokenize, 'decode': r_decode}
