"""Case tables, inputs and tolerances shared by tests/test_gpu_attn_cores.py (the kernels against float64) and
tests/test_attn_cores_host.py (the same inputs on the CPU: can the bound see a wrong key, a skipped belief projection, ...?).

A case is a dict; `form` is the kernel form its launcher must pick (d4_debug_last_form).  Inputs are seeded normals (gamma ~ 0.2 N,
gate / mix logits ~ N), generated on the CPU from the case's position in its table, so both files see the same numbers.

The tolerance.  E32[family] is the largest error of the float32 evaluation of attn_core_ref against its float64 evaluation over the
family's cases, max-abs relative to the output's max-abs, measured on the CPU and recorded here with a quarter of headroom for another
CPU's summation order (test_attn_cores_host.py asserts it still holds).  The kernels differ from the float32 reference only in
summation order and the device's tanhf / expf / sincosf, so the GPU bound is FACTOR x E32, and the host test demands that every
mutation of attn_core_ref.MUTATIONS moves an output by at least 10 x that bound."""
import math

import torch

import attn_core_ref as R

FACTOR = 8
E32 = {'small_attn': 1.2e-6, 'pool_mix': 6.0e-7, 'time': 6.6e-6}
BOUND = {f: FACTOR * e for f, e in E32.items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _n(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


# ------------------------------------------------------------------------------------------------------------------- small_attn
def _sa(name, form, nq, nk, dh=64, G=2, H=2, vres=0, ms=0, belief=0, clamp=50., align='ok', restrict=None, q0=0, ob=0, gate=1):
    return dict(name=name, form=form, nq=nq, nk=nk, dh=dh, G=G, H=H, vres=vres, ms=ms, belief=belief, clamp=clamp, align=align,
                restrict=restrict, q0=q0, ob=ob, gate=gate)


def _small_attn_cases():
    cs, i = [], 0
    # within-frame self attention over 8..16 tokens: the matrix-pipe form and the LDS-staged forms
    for n in (8, 11, 15, 16):
        for dh, align in ((64, 'ok'), (64, 'ptr'), (64, 'stride'), (32, 'ok'), (16, 'ok')):
            form = 'attn_mfma_kernel<1,1>' if (dh, align) == (64, 'ok') else f'space_attn_kernel<{dh}>'
            cs.append(_sa(f'space-n{n}-dh{dh}-{align}', form, n, n, dh, G=2 + i % 2, H=1 + i % 3, vres=i % 2, ms=(0, 1, n // 2)[i % 3], belief=1,
                          clamp=50. if (i // 2) % 2 == 0 else 3., align=align, ob=int(i % 4 == 1)))
            i += 1
    for dh, align in ((64, 'ok'), (64, 'ptr'), (32, 'ok')):
        form = 'attn_mfma_kernel<1,1>' if (dh, align) == (64, 'ok') else f'space_attn_kernel<{dh}>'
        for last in (0, 1):
            cs.append(_sa(f'space-restrict-dh{dh}-{align}-last{last}', form, 11, 11, dh, G=3, H=2, vres=1, ms=1, belief=1, align=align,
                          restrict=(1, 6, last), ob=int(align == 'ok' and dh == 64)))
    # small cross forms
    pairs = [((1, 5), '1,1', 16), ((7, 7), '1,1', 16), ((16, 17), '1,2', 32), ((16, 32), '1,2', 32), ((3, 33), '1,4,2', 64), ((16, 64), '1,4,2', 64),
             ((17, 16), '2,1', 16), ((32, 9), '2,1', 16), ((33, 16), '4,1', 16), ((64, 16), '4,1', 16)]
    for j, ((nq, nk), mf, nkm) in enumerate(pairs):
        self_ = nq == nk
        kw = dict(G=3, H=1 + 2 * (j % 2), vres=j % 2, ms=int(j % 3 == 1), belief=int(self_), clamp=3. if j % 4 == 3 else 50., gate=int(j != 4))
        cs.append(_sa(f'cross-{nq}x{nk}-mfma', f'attn_mfma_kernel<{mf}>', nq, nk, 64, q0=int(j in (4, 7)), ob=int(j % 3 == 0), **kw))
        cs.append(_sa(f'cross-{nq}x{nk}-dh64-mis', f'small_attn_kernel<{nkm},64>', nq, nk, 64, align=('ptr', 'stride')[j % 2], q0=int(j == 2), ob=int(j % 5 == 0), **kw))
        cs.append(_sa(f'cross-{nq}x{nk}-dh32', f'small_attn_kernel<{nkm},32>', nq, nk, 32, **kw))
        cs.append(_sa(f'cross-{nq}x{nk}-dh16', f'small_attn_kernel<{nkm},16>', nq, nk, 16, **kw))
    cs.append(_sa('generic-40x40', 'small_attn_kernel<64,64>', 40, 40, 64, G=2, H=3, vres=1, ms=2))
    # wide kernel
    for j, nk in enumerate((65, 67, 100, 128, 129, 160)):
        cs.append(_sa(f'wide-self-{nk}', 'attn_wide_kernel', nk, nk, 64, G=2, H=1 + j % 2, vres=j % 2, ms=(0, 3)[j % 2], belief=1, clamp=3. if j == 2 else 50.))
        cs.append(_sa(f'wide-5x{nk}', 'attn_wide_kernel', 5, nk, 64, G=2, H=2, vres=(j + 1) % 2, ms=(3, 0)[j % 2], ob=int(j == 0)))
    cs.append(_sa('wide-self-17', 'attn_wide_kernel', 17, 17, 64, G=3, H=2, vres=1, ms=3, belief=1))
    cs.append(_sa('wide-self-64', 'attn_wide_kernel', 64, 64, 64, G=2, H=1, vres=0, ms=0, belief=1, clamp=3.))
    for k, c in enumerate(cs):
        c['seed'] = 1000 + k
    return cs


SMALL_ATTN = _small_attn_cases()


def small_attn_inputs(c):
    g = _gen(c['seed'])
    G, H, nq, nk, dh = c['G'], c['H'], c['nq'], c['nk'], c['dh']
    d = dict(q=_n(g, 1 if c['q0'] else G, H, nq, dh), k=_n(g, G, H, nk, dh), v=_n(g, G, H, nk, dh), gamma=_n(g, H, dh, scale=0.2),
             gate=_n(g, G, H, nq) if c['gate'] else None, vres=None, mix=None)
    if c['vres']:
        d['vres'], d['mix'] = _n(g, G, H, nk, dh), _n(g, G, H, nk)
    return d


def small_attn_expect(c, d, dtype=torch.float64, mut=()):
    lo, hi, last = c['restrict'] or (0, 0, 1)
    return R.small_attn_ref(d['q'], d['k'], d['v'], d['gamma'], d['gate'], d['vres'], d['mix'], clamp=c['clamp'], mask_special=c['ms'],
                            belief=c['belief'], q_lo=lo, q_hi=hi, q_last=last, dtype=dtype, mut=mut)


def small_attn_mutations(c):
    m = ['drop_newest', 'drop_oldest', 'gamma_only']
    if c['nk'] == 1:
        m = ['gamma_only']
    if c['ms'] > 0 and c['nq'] > c['ms']:
        m.append('extra_key')
        if not (c['restrict'] and not c['restrict'][2]):      # (the row whose mask moves is outside that restricted query set)
            m.append('mask_row')
    if c['belief']:
        m.append('no_belief')
    if c['vres']:
        m.append('no_vres')
    if c['dh'] != 64:
        m.append('scale64')
    return m


# ------------------------------------------------------------------------------------------------------------------- pool_mix
def _pm(D, L, M, kb, i):
    rows = M <= 2048 and D <= 512
    it = 1 if D <= 256 else 2 if D <= 512 else 4
    form = ('pool_mix_rows_kernel' if rows else 'pool_mix_kernel') + f'<{it}' + (',bf16>' if kb else '>')
    return dict(name=f'pool-D{D}-L{L}-M{M}-' + ('bf16' if kb else 'f32'), form=form, D=D, L=L, M=M, kb=kb, x_last=int(i % 2 == 0), qb=int(kb and i % 3 != 0),
                hb=int(kb and (i // 2) % 2 == 0), ub=int(i % 3 == 0), eps=1.1920929e-07)


def _pool_cases():
    pairs = [(64, 1), (64, 5), (64, 33), (96, 3), (96, 17), (96, 64), (256, 4), (256, 16), (256, 33), (320, 1), (320, 5), (320, 64), (512, 3), (512, 16),
             (512, 17), (768, 4), (768, 5), (768, 33), (1024, 1), (1024, 17), (1024, 64),
             (64, 34), (320, 35), (96, 18), (512, 19), (768, 18), (1024, 35)]          # (second rounds of the block-per-row form at every L % 4)
    cs = []
    for i, (D, L) in enumerate(pairs):
        for kb in (0, 1):
            cs.append(_pm(D, L, (1, 5)[(i + kb) % 2], kb, i + kb))
    for i, (D, M, kb) in enumerate([(64, 2048, 0), (64, 2049, 0), (64, 2049, 1), (64, 2048, 1), (320, 2049, 0), (320, 2049, 1), (320, 2048, 0)]):
        cs.append(_pm(D, 5, M, kb, i))
    for k, c in enumerate(cs):
        c['seed'] = 2000 + k
    return cs


POOL_MIX = _pool_cases()


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def pool_inputs(c):
    """fp32 operands; with bf16 keys (`kb`) the kernel is handed bf16 images of k (and q, hid where the case says so)."""
    g = _gen(c['seed'])
    D, L, M = c['D'], c['L'], c['M']
    d = dict(q=_n(g, M, 256), k=_n(g, L, M, 256), hid=_n(g, L, M, D) * (0.5 + torch.rand(L, M, 1, generator=g) * 2), gate_w=_n(g, 4, D, scale=D ** -0.5 * 2),
             gamma=_n(g, 4, 64, scale=0.2), x=None if c['x_last'] else _n(g, M, D))
    return d


def pool_expect(c, d, dtype=torch.float64, mut=()):
    """The reference on the values the chosen form reads: bf16-rounded keys / queries / hiddens where their bf16 image is what the kernel reads
    (the hiddens' image is read by the wave-per-row form only: PoolMixArgs::hid_b)."""
    k = bf16_round(d['k']) if c['kb'] else d['k']
    q = bf16_round(d['q']) if c['qb'] else d['q']
    hid = bf16_round(d['hid']) if (c['hb'] and c['form'].startswith('pool_mix_kernel')) else d['hid']
    x = hid[-1] if c['x_last'] else d['x']
    return R.pool_mix_ref(q, x, d['gate_w'], k, hid, d['gamma'], eps=c['eps'], dtype=dtype, mut=mut)


def pool_mutations(c):
    m = ['no_rms']
    if c['L'] > 1:                                           # (the softmax over a single hidden is 1 whatever its score)
        m += ['gamma_only', 'drop_newest', 'drop_oldest']
    if c['M'] > 1 or c['L'] > 1:
        m.append('gate_row')
    return m


# ------------------------------------------------------------------------------------------------------------------- time decode
TCAP = 256


def _td(kind, H, dh, Tq, t0, align='ok', cb=0, ob=0, clamp=50., mode=0, t0_dev=None):
    """kind: 'append' (mode 1 alone), 'decode' (one frame: mode 0 against modes 1 + 2), 'frames' (several frames, mode 0), 't0dev'."""
    al = align == 'ok'
    if dh == 64:
        kv = 'time_kv_append4_kernel' if (H % 4 == 0 and al) else 'time_kv_append_kernel<64>'
    else:
        kv = f'time_kv_append_kernel<{dh}>'
    t_eff = t0                                              # the launcher picks by the host-side t0
    if dh != 64 or not al:
        at = f'time_attn_kernel<{dh}>'
    elif Tq > 1:
        at = 'time_attn64_kernel<true>'
    elif H % 4 == 0 and t_eff < 16:
        at = 'time_attn64_few_kernel<8>' if t_eff < 8 else 'time_attn64_few_kernel<16>'
    else:
        at = 'time_attn64_kernel<false>'
    fused = dh == 64 and al and Tq == 1
    at0 = at[:-1] + ',append>' if fused else at              # mode 0: the appending form where there is one
    return dict(name=f'{kind}-H{H}-dh{dh}-Tq{Tq}-t{t0}' + (f'-dev{t0_dev}' if t0_dev is not None else '') + f'-{align}' + ('-cb' if cb else ''), kind=kind,
                H=H, dh=dh, Tq=Tq, t0=t0, align=align, cb=cb, ob=ob, clamp=clamp, kv_form=kv, attn_form=at, attn_form0=at0, fused=fused, t0_dev=t0_dev,
                B=2, S=3, cache_batch=3 if cb else 2, cache_S=4 if cb else 3)


def _time_cases():
    cs = [_td('append', 4, 64, 1, 0), _td('append', 8, 64, 5, 63, cb=1), _td('append', 4, 64, 5, 200), _td('append', 8, 64, 1, 200),
          _td('append', 1, 64, 1, 63), _td('append', 3, 64, 5, 0, cb=1), _td('append', 4, 64, 5, 200, align='ptr'), _td('append', 4, 64, 1, 0, align='stride', cb=1),
          _td('append', 3, 64, 1, 200, align='ptr'),
          _td('append', 2, 32, 5, 63, cb=1), _td('append', 4, 32, 1, 200), _td('append', 1, 32, 5, 0),
          _td('append', 3, 16, 5, 0), _td('append', 4, 16, 1, 200, cb=1), _td('append', 2, 16, 5, 63)]
    for i, t0 in enumerate((0, 1, 7, 8, 15, 16, 63, 64, 65, 127, 128, 200)):
        cs.append(_td('decode', 4, 64, 1, t0, cb=int(i % 3 == 0), ob=int(i % 2 == 0), clamp=3. if i % 4 == 1 else 50.))
        cs.append(_td('decode', 3, 64, 1, t0, cb=int(i % 3 == 1), ob=int(i % 2 == 1), clamp=3. if i % 4 == 2 else 50.))
    for i, t0 in enumerate((0, 65, 200)):
        cs.append(_td('decode', 2, 32, 1, t0, cb=int(i == 1), ob=int(i == 2), clamp=3. if i == 0 else 50.))
        cs.append(_td('decode', 3, 16, 1, t0, cb=int(i == 2), clamp=3. if i == 1 else 50.))
        cs.append(_td('decode', 4, 64, 1, t0, align='ptr', cb=int(i == 0), clamp=3. if i == 2 else 50.))
    cs.append(_td('decode', 4, 64, 1, 65, align='stride'))
    for i, Tq in enumerate((2, 4, 5, 9)):
        for j, t0 in enumerate((0, 60, 126)):
            cs.append(_td('frames', (4, 3)[(i + j) % 2], 64, Tq, t0, cb=int((i + j) % 3 == 0), ob=int(j == 1), clamp=3. if (i, j) in ((2, 1), (3, 2)) else 50.))
    cs += [_td('frames', 2, 32, 5, 60), _td('frames', 4, 64, 5, 60, align='ptr')]
    cs += [_td('t0dev', 4, 64, 1, 16, t0_dev=130, cb=1), _td('t0dev', 4, 64, 1, 3, t0_dev=6), _td('t0dev', 4, 64, 1, 9, t0_dev=12),
           _td('t0dev', 3, 64, 1, 3, t0_dev=6), _td('t0dev', 2, 32, 1, 16, t0_dev=130), _td('t0dev', 4, 64, 3, 16, t0_dev=130)]
    for k, c in enumerate(cs):
        c['seed'] = 3000 + k
    return cs


TIME = _time_cases()


def time_pos(c):
    """The frame offset the result must be computed at: the device value where there is one."""
    return c['t0'] if c['t0_dev'] is None else c['t0_dev']


def time_inputs(c):
    """hist_*: the t0 earlier frames (prefilled into the cache by one append call), proj / vres: the Tq frames of the call under test."""
    g = _gen(c['seed'])
    B, S, H, dh, Tq = c['B'], c['S'], c['H'], c['dh'], c['Tq']
    t0 = 0 if c['kind'] == 'append' else time_pos(c)         # (the append alone reads no history: its cases start from an empty cache)
    hd, nc = H * dh, 3 * H * dh + 2 * H
    inv = torch.zeros(32)
    inv[:dh // 2] = 1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))
    return dict(proj=_n(g, B, Tq, S, nc), vres=_n(g, B, Tq, S, hd), gamma=_n(g, H, dh, scale=0.2), inv_freq=inv,
                hist_proj=_n(g, B, t0, S, nc) if t0 else None, hist_vres=_n(g, B, t0, S, hd) if t0 else None)


def time_expect(c, d, dtype=torch.float64, mut=(), fill=None):
    """-> (cache after the call [2, cache_batch, cache_S, H, TCAP, dh] with NaN where nothing is written, out [B, Tq, S, hd]).
    `fill`: a value tensor for the never-written cache positions (the host test's 'extra_key' mutation reads one)."""
    H, dh, t0 = c['H'], c['dh'], time_pos(c)
    cache = torch.full((2, c['cache_batch'], c['cache_S'], H, TCAP, dh), math.nan, dtype=dtype)
    amut = [m for m in mut if m in ('no_vres', 'scale64', 'gamma_only', 'rot_off_k')]
    if d['hist_proj'] is not None:
        R.time_append_ref(d['hist_proj'], d['hist_vres'], d['gamma'], d['inv_freq'], cache, t0=0, H=H, dh=dh, dtype=dtype, mut=amut)
    R.time_append_ref(d['proj'], d['vres'], d['gamma'], d['inv_freq'], cache, t0=t0, H=H, dh=dh, dtype=dtype, mut=amut)
    src = cache if fill is None else torch.where(cache.isnan(), fill.to(dtype), cache)
    out = R.time_attn_ref(d['proj'], d['inv_freq'], src, t0=t0, H=H, dh=dh, clamp=c['clamp'], dtype=dtype, mut=mut)
    return cache, out


def time_scale(c, cache, out):
    """What an error of `out` is measured against: the output's max-abs — except for the single frame at position 0, where the one key's value
    IS the own value, the belief projection cancels the whole output (it is rounding noise around 0) and the scale is that value row's."""
    if time_pos(c) == 0 and c['Tq'] == 1:
        return cache[1, :c['B'], :c['S'], :, 0].abs().max().item()
    return out.abs().max().item()


def time_mutations(c):
    if c['kind'] == 'append':                                # (the written cache rows are its only output)
        return ['gamma_only', 'no_vres', 'rot_off_k'] + (['scale64'] if c['dh'] != 64 else [])
    m = ['gamma_only', 'no_vres', 'no_belief', 'extra_key']
    if time_pos(c) + c['Tq'] > 1:
        m += ['drop_newest', 'drop_oldest', 'rot_off']
    if c['dh'] != 64:
        m.append('scale64')
    return m
