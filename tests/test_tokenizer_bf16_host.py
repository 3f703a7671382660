"""Host side of VideoTokenizer(matmul_dtype='bf16'): the option, its way through the configuration, checkpoints and copies, the new
operator symbols, and the yardstick of the GPU tests — the oracle's own bf16 envelope per case (tests/tokenizer_bf16_cases.py).

There is no mutation test: an emulation that ALSO rounds the residual stream to bf16 after every block moves the oracle by 1.3 .. 1.8 E_max at the
cases' sizes, inside 3 E_max + 1e-4 on every case and metric (figures in DESIGN.md 27), so no case of this size separates the two contracts."""
import copy
import math

import pytest
import torch

import tokenizer_bf16_cases as cases
from dreamer4_amd import DynamicsWorldModel, VideoTokenizer, _lib

KW = dict(dim=32, dim_latent=8, patch_size=4, image_height=16, image_width=24, num_latent_tokens=6, encoder_depth=1, decoder_depth=1, attn_heads=2)


def test_the_default_is_fp32_and_the_option_is_validated():
    tok = VideoTokenizer(**KW)
    assert tok.matmul_dtype == 'fp32' and tok._config[1]['matmul_dtype'] == 'fp32'
    assert VideoTokenizer(**KW, matmul_dtype='fp32').matmul_dtype == 'fp32'
    assert VideoTokenizer(**KW, matmul_dtype='bf16').matmul_dtype == 'bf16'
    for bad in ('fp16', 'bfloat16', None, 1, 'fp32_fp16x2'):
        with pytest.raises(ValueError, match='matmul_dtype'):
            VideoTokenizer(**KW, matmul_dtype=bad)


@pytest.mark.parametrize('mode', [1, 2])
def test_make_config_sets_matmul_bf16_without_a_device(mode):
    plain, b = VideoTokenizer(**KW), VideoTokenizer(**KW, matmul_dtype='bf16')
    c0, c1 = plain._make_config(mode, (2, 3)), b._make_config(mode, (2, 3))
    assert c0.matmul_bf16 == 0 and c1.matmul_bf16 == 1
    assert (c0.mode, c0.max_batch, c0.max_frames, c0.max_parallel_frames) == (mode, 2, 3, 3)
    assert c0.depth == 1 and c0.dim == 32 and c0.pool_heads == 4 and c0.wide_frames == 0
    # every other field is the same: the option touches matmul_bf16 alone
    for name, _ in _lib.Config._fields_:
        if name not in ('matmul_bf16', 'num_discrete_actions'):
            assert getattr(c0, name) == getattr(c1, name), name


def test_independent_of_the_other_options():
    for extra in (dict(wide_frames=True), dict(wide_frames=True, attn_products='bf16'), dict(train_wide_frames=True)):
        tok = VideoTokenizer(**KW, matmul_dtype='bf16', **extra)
        c = tok._make_config(1, (1, 1))
        assert c.matmul_bf16 == 1 and c.wide_frames == (3 if extra.get('attn_products') == 'bf16' else int(bool(extra.get('wide_frames'))))
        assert VideoTokenizer(**KW, **extra)._make_config(2, (1, 1)).matmul_bf16 == 0


def test_config_checkpoint_and_deepcopy_keep_the_option(tmp_path):
    tok = VideoTokenizer(**KW, matmul_dtype='bf16')
    assert tok._config[1]['matmul_dtype'] == 'bf16'
    path = tmp_path / 'tok.pt'
    tok.save(path)
    back = VideoTokenizer.init_and_load(path)
    assert back.matmul_dtype == 'bf16' and back._make_config(1, (1, 1)).matmul_bf16 == 1
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in tok.state_dict().items())
    # a checkpoint written without the option loads as fp32
    plain = VideoTokenizer(**KW)
    plain.save(path)
    assert VideoTokenizer.init_and_load(path).matmul_dtype == 'fp32'
    assert VideoTokenizer.init_and_load(path, matmul_dtype='bf16').matmul_dtype == 'bf16'
    dup = copy.deepcopy(tok)
    assert dup.matmul_dtype == 'bf16' and dup._engines == {} and dup._make_config(2, (1, 1)).matmul_bf16 == 1


def test_a_world_model_keeps_its_tokenizers_option(tmp_path):
    tok = VideoTokenizer(**KW, matmul_dtype='bf16')
    m = DynamicsWorldModel(dim=64, dim_latent=8, depth=2, time_block_every=2, attn_heads=2, num_discrete_actions=4, video_tokenizer=tok)
    assert m.video_tokenizer.matmul_dtype == 'bf16'
    assert getattr(m, 'matmul_dtype', 'fp32') == 'fp32', "the world model's own option is independent"
    path = tmp_path / 'wm.pt'
    m.save(path)
    assert DynamicsWorldModel.init_and_load(path).video_tokenizer.matmul_dtype == 'bf16'


def test_the_new_operator_is_declared():
    assert 'd4_pack_tokens_bf16' in _lib.SYMBOLS
    res, args = _lib.SYMBOLS['d4_pack_tokens_bf16']
    base = _lib.SYMBOLS['d4_pack_tokens'][1]
    assert len(args) == len(base) + 2, 'd4_pack_tokens plus the two image pointers'
    import os
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'd4hip.h')).read()
    assert 'int d4_pack_tokens_bf16(' in header and header.index('int d4_pack_tokens_bf16(') > header.index('int d4_recon_loss_fwd_bwd('), 'appended'


@pytest.mark.parametrize('name', list(cases.CASES))
def test_the_envelope_governs_the_bound(name):
    """E_max (oracle fp32 vs oracle with bf16-rounded Linear operands) is finite and at least ten times the fp32 tests' tolerance."""
    E = cases.reference(name)['E']
    for out in ('decode', 'tokenize'):
        for metric in cases.METRICS:
            e = E[out][metric]
            print(f'case {name} {out} {metric}: E_max {e:.3e}  bound {cases.bound(e):.3e}')
            assert math.isfinite(e) and e >= 10 * cases.FP32_TOL, (name, out, metric, e)
            assert e < 0.1, 'an envelope of ten per cent would bound nothing'


def test_case_e_shares_case_ds_oracle():
    assert cases.reference('E') is cases.reference('D')
    assert cases.CASES['E']['kw']['attn_products'] == 'bf16' and cases.CASES['E']['kw']['wide_frames']
