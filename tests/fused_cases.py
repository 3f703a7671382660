"""Case tables, inputs and tolerances shared by tests/test_gpu_fused_launches.py (the per-frame fused tails of csrc/frame_fused.hip against
float64) and tests/test_fused_launches_host.py (the same inputs on the CPU: can the bound see a swapped weight tile, a shifted row, a wrong
compact rank, ...?).  The scheme is attn_core_cases.py's, whose input generators and FACTOR are used here.

Inputs are seeded CPU normals; the projection weights are scaled by 1 / sqrt(K), so the projected term and the residual are both O(1) and
neither hides the other.

The tolerance.  E32[family] is the largest error of the float32 evaluation of fused_ref against its float64 evaluation over the family's
cases (max-abs relative to the output's max-abs, the compact copy included), measured on the CPU and recorded with a quarter of headroom;
the GPU bound is FACTOR x E32.  Measured (the host test prints them): frame_attn_out 2.13e-7, attn_out_cols 1.58e-7, frame_pool 5.02e-7."""
import torch

import attn_core_cases as K
import fused_ref as F

FACTOR = K.FACTOR
E32 = {'frame_attn_out': 2.7e-7, 'attn_out_cols': 2.0e-7, 'frame_pool': 6.3e-7}
BOUND = {f: FACTOR * e for f, e in E32.items()}
H, DH, HD = 8, 64, 512                  # the per-frame attention tails: 8 heads x 64
PH, HP = 4, 256                         # the pool tails: 4 heads x 64
C2S = {'none': None, 'agent': (1, 5, 1), 'noagent': (1, 5, 0), 'all': 'all'}


def _c2(c):
    v = C2S[c['c2']]
    return (0, c['S'], 0) if v == 'all' else v


def keep_rows(c):
    c2 = _c2(c)
    return 0 if c2 is None else c2[1] - c2[0] + c2[2]


# ------------------------------------------------------------------------------------------------------------------- frame_attn_out
def _fa(frames, S, D, vres, ms, clamp, c2, pad, belief=1):
    return dict(name=f'fao-F{frames}-S{S}-D{D}-v{vres}-ms{ms}-cl{clamp:g}-{c2}-pad{pad}' + ('' if belief else '-nobelief'), frames=frames, S=S, D=D, vres=vres,
                ms=ms, clamp=clamp, c2=c2, pad=pad, belief=belief)


def _frame_attn_out_cases():
    # every value of the issue's lists at least once: frames 192 / 193 / 1024, S 1 / 8 / 11 / 15 / 16 (2 at 1024 frames), D 256 / 288 / 512 /
    # 544 (8, 9, 16, 17 units on 8 waves), value residual, special-token mask, clamp 50 / 3, the four compactions, padded leading dimensions
    cs = [_fa(192, 15, 512, 1, 1, 50., 'agent', 0), _fa(192, 15, 512, 0, 0, 3., 'none', 4), _fa(193, 11, 288, 1, 1, 50., 'noagent', 4),
          _fa(193, 16, 544, 0, 1, 3., 'all', 0), _fa(192, 1, 256, 1, 0, 50., 'all', 4), _fa(192, 1, 512, 0, 0, 50., 'none', 0),
          _fa(192, 8, 256, 0, 1, 50., 'agent', 4), _fa(193, 8, 544, 1, 0, 3., 'noagent', 0), _fa(192, 16, 288, 1, 0, 50., 'agent', 0),
          _fa(193, 16, 512, 1, 1, 50., 'noagent', 4), _fa(192, 11, 544, 0, 0, 50., 'agent', 4), _fa(193, 15, 256, 1, 1, 3., 'all', 0),
          _fa(1024, 2, 512, 1, 1, 50., 'all', 0), _fa(1024, 2, 288, 0, 0, 3., 'none', 4), _fa(192, 15, 288, 0, 1, 50., 'none', 0),
          _fa(193, 11, 512, 0, 0, 50., 'agent', 0),
          # a single token with the belief projection on attends to itself and the projection cancels its whole output: the output projection
          # of a one-token frame is seen by this case only
          _fa(192, 1, 288, 1, 0, 50., 'all', 0, belief=0)]
    for i, c in enumerate(cs):
        c.update(seed=5000 + i, G=c['frames'], H=H, nq=c['S'], nk=c['S'], dh=DH, q0=0, gate=1)
    return cs


FRAME_ATTN_OUT = _frame_attn_out_cases()


# ------------------------------------------------------------------------------------------------------------------- attn_out_cols
def _ac(groups, S, D, ldw, vres, ms, clamp, c2, pad, belief=1):
    return dict(name=f'aoc-G{groups}-S{S}-D{D}-ldw{ldw}-v{vres}-ms{ms}-{c2}-pad{pad}' + ('' if belief else '-nobelief'), frames=groups, S=S, D=D, ldw=ldw, vres=vres,
                ms=ms, clamp=clamp, c2=c2, pad=pad, belief=belief)


def _attn_out_cols_cases():
    cs = [_ac(1, 11, 512, 512, 1, 1, 50., 'agent', 0), _ac(4, 16, 272, 516, 0, 1, 3., 'all', 4), _ac(4, 1, 16, 512, 1, 0, 50., 'all', 0),
          _ac(1, 16, 16, 516, 0, 0, 50., 'none', 4), _ac(4, 11, 272, 512, 1, 1, 50., 'noagent', 0), _ac(1, 1, 512, 516, 0, 0, 3., 'none', 0),
          _ac(4, 11, 512, 516, 1, 0, 50., 'agent', 4), _ac(4, 1, 272, 516, 1, 0, 50., 'all', 0, belief=0)]
    for i, c in enumerate(cs):
        c.update(seed=6000 + i, G=c['frames'], H=H, nq=c['S'], nk=c['S'], dh=DH, q0=0, gate=1)
    return cs


ATTN_OUT_COLS = _attn_out_cols_cases()


def attn_inputs(c):
    """small_attn inputs of the frame (attn_core_cases) + Wo [D, 512] / sqrt(512) + resid [frames, S, D]"""
    d = K.small_attn_inputs(c)
    g = K._gen(c['seed'] + 500)
    d['Wo'] = K._n(g, c['D'], HD, scale=HD ** -0.5)
    d['resid'] = K._n(g, c['frames'], c['S'], c['D'])
    return d


def attn_expect(c, d, dtype=torch.float64, mut=()):
    return F.frame_attn_out_ref(d['q'], d['k'], d['v'], d['gamma'], d['gate'], d['vres'], d['mix'], d['Wo'], d['resid'], clamp=c['clamp'],
                                mask_special=c['ms'], belief=c['belief'], c2=_c2(c), dtype=dtype, mut=mut)


def _out_mutations(c):
    m = ['no_resid']
    if c['S'] > 1 or not c.get('belief'):                    # (the belief projection cancels a one-token frame's attention output: nothing is projected)
        m.append('k4_swap')
        if c['D'] >= 32:
            m.append('tile_swap')
    if c['S'] > 1:
        m.append('row_shift')
    if keep_rows(c) > 1:
        m.append('rank_off')
    if _c2(c) is not None and _c2(c)[2]:
        m.append('last_missing')
    return m


def attn_mutations(c):
    m = _out_mutations(c) + (['no_belief'] if c['belief'] else [])
    if c['S'] - c['ms'] > 1:                                 # (an ordinary query keeps a key to attend to)
        m.append('drop_newest')
    if c['vres'] and (c['S'] > 1 or not c['belief']):
        m.append('no_vres')
    if c['ms'] > 0 and c['S'] > c['ms']:
        m.append('extra_key')
    return m


# ------------------------------------------------------------------------------------------------------------------- frame_pool (+ tail)
def _fp(frames, S, L, c2, pad, x_last):
    return dict(name=f'pool-F{frames}-S{S}-L{L}-{c2}-pad{pad}-x{x_last}', frames=frames, S=S, L=L, D=512, M=frames * S, c2=c2, pad=pad, x_last=x_last,
                eps=1.1920929e-07)


def _frame_pool_cases():
    # S 1 / 11 / 16 at 192 frames; L 1 / 5 / 32 / 33 / 64: both instances of frame_pool_kernel on either side of their switch (few token rows
    # at the long stacks: the hiddens stay under 100 MB); 1024 frames of 2 tokens
    cs = [_fp(192, 11, 5, 'agent', 0, 1), _fp(192, 16, 5, 'noagent', 4, 0), _fp(192, 1, 1, 'all', 0, 1), _fp(192, 16, 1, 'none', 4, 1),
          _fp(192, 3, 32, 'all', 4, 0), _fp(192, 3, 33, 'all', 0, 1), _fp(192, 1, 33, 'none', 0, 0), _fp(192, 3, 64, 'none', 4, 1),
          _fp(192, 11, 1, 'agent', 4, 0), _fp(1024, 2, 1, 'all', 0, 0), _fp(192, 1, 32, 'all', 4, 1)]
    for i, c in enumerate(cs):
        c['seed'] = 7000 + i
    return cs


FRAME_POOL = _frame_pool_cases()


def pool_inputs(c):
    """pool_mix inputs (attn_core_cases) + Wv [256, D] / sqrt(D) + Wo [D, 256] / 16 + resid [frames, S, D]"""
    d = K.pool_inputs(c)
    g = K._gen(c['seed'] + 500)
    D = c['D']
    d['Wv'] = K._n(g, HP, D, scale=D ** -0.5)
    d['Wo'] = K._n(g, D, HP, scale=HP ** -0.5)
    d['resid'] = K._n(g, c['frames'], c['S'], D)
    return d


def pool_expect(c, d, dtype=torch.float64, mut=()):
    x = d['hid'][-1] if c['x_last'] else d['x']
    return F.frame_pool_ref(d['q'], x, d['gate_w'], d['k'], d['hid'], d['gamma'], d['Wv'], d['Wo'], d['resid'], eps=c['eps'], frames=c['frames'],
                            c2=_c2(c), dtype=dtype, mut=mut)


def pool_mutations(c):
    m = _out_mutations(c) + ['head_swap', 'no_rms']
    if c['L'] > 1:
        m.append('drop_newest')
    return m
