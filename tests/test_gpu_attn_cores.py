"""GPU: every kernel form of the inference attention launchers (csrc/attn.hip: small_attn, pool_mix, time_kv_append / time_attn /
time_attn_append) against the plain float64 references of tests/attn_core_ref.py, one operator call per case through the C-ABI test entry
points d4_small_attn / d4_pool_mix / d4_time_attn_decode.

A case (tests/attn_core_cases.py) asserts
  * the form: d4_debug_last_form names the kernel the case was written for;
  * the values: max |out - float64| <= BOUND[family] x max |float64|;
  * the bf16 copy (where requested): bit for bit the round-to-nearest-even bf16 of the fp32 output;
  * untouched memory: every output, cache and guard element the operation must not write is still the NaN it was pre-filled with — cache
    positions past the newest frame, cache rows of unused batch / token slots, output rows outside a restricted query set, the gaps of
    padded rows.  (Operand gaps are NaN too, so a kernel that reads past a row, or a key past `pos`, poisons its output.)
The last test asserts that the forms seen over the module are the library's full list per family (d4_debug_forms): a form added later
without a case here fails the suite.

Tolerance (attn_core_cases.py; derivation in DESIGN.md): E32 = float32 against float64 evaluation of the same reference on the CPU, worst
case of the family, recorded with 25 % headroom; the GPU bound is 8 x E32, relative to the output's max-abs:
    family       measured E32   recorded E32   bound (8 x)
    small_attn   9.2e-7         1.2e-6         9.6e-6
    pool_mix     4.8e-7         6.0e-7         4.8e-6
    time         5.3e-6         6.6e-6         5.3e-5      (most of it is the rotary angle pos * f, formed in float32 at pos <= 209)
The time decode of the single frame at position 0 is measured against its value row's max-abs: the belief projection cancels that output."""
import ctypes as C
import math

import pytest
import torch

import attn_core_cases as K
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of NaN in front of and behind every buffer (256 bytes: keeps 16-byte alignment)
SEEN = {'small_attn': set(), 'pool_mix': set(), 'time_kv_append': set(), 'time_attn': set()}
WORST = {'small_attn': (0., ''), 'pool_mix': (0., ''), 'time': (0., '')}
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_form(lib, family):
    f = lib.d4_debug_last_form(family.encode())
    assert f is not None, f'no {family} form recorded'
    SEEN[family].add(f.decode())
    return f.decode()


def note(family, name, err, bound):
    print(f'{family} {name}: err {err:.3e} (bound {bound:.3e})')
    if err > WORST[family][0]:
        WORST[family] = (err, name)


class Buf:
    """A flat device buffer between two NaN guards, NaN in every gap; `ptr` points `off` elements past the front guard."""

    def __init__(self, size, off=0, dtype=torch.float32):
        self.off, self.size, self.dtype = off, size, dtype
        self.host = torch.full((GUARD + off + size + GUARD,), math.nan, dtype=torch.float32).to(dtype)
        self.dev = None

    def view(self, shape, strides):
        return self.host.as_strided(shape, strides, GUARD + self.off)

    def upload(self):
        self.dev = self.host.to(DEV)
        return self

    @property
    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + self.dev.element_size() * (GUARD + self.off))

    def clone(self):
        b = Buf.__new__(Buf)
        b.off, b.size, b.dtype, b.host, b.dev = self.off, self.size, self.dtype, self.host, self.dev.clone()
        return b


def rows_buf(x, item_stride, group_stride=None, off=0):
    """x [G, n, w] (CPU fp32) laid out with the given strides (group_stride 0: one shared group) -> (Buf, group stride, item stride)"""
    G, n, w = x.shape
    gs = n * item_stride if group_stride is None else group_stride
    b = Buf((G - 1) * gs + (n - 1) * item_stride + w, off)
    b.view((G, n, w), (gs, item_stride, 1)).copy_(x)
    return b.upload(), (gs if G > 1 or group_stride != 0 else 0), item_stride


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def check_image(got, want, bound, scale=None):
    """got: the device buffer as written (fp32, flat, guards included); want: the same image on the CPU in float64, NaN wherever nothing may
    be written.  -> error relative to max |want| (or `scale`)."""
    got = got.cpu()
    keep = want.isnan()
    assert got[keep].isnan().all(), f'{int((~got[keep].isnan()).sum())} elements written that the operation must not touch'
    g, w = got[~keep].double(), want[~keep]
    assert not g.isnan().any(), 'NaN in the output (an operand gap, an unwritten cache row or a key past the newest frame was read, or a row was not written)'
    err = ((g - w).abs().max() / (w.abs().max() if scale is None else scale)).item()
    assert err <= bound, f'error {err:.3e} above the bound {bound:.3e}'
    return err


def check_bf16_copy(out, out_b):
    """out_b is the round-to-nearest-even bf16 image of out, bit for bit; NaN (untouched) exactly where out is."""
    o, b = out.dev.cpu(), out_b.dev.cpu()
    keep = o.isnan()
    assert b[keep].isnan().all()
    assert torch.equal(bits(o[~keep].to(torch.bfloat16)), bits(b[~keep]))


# ------------------------------------------------------------------------------------------------------------------- small_attn
def small_attn_call(lib, c, d, *, restrict=None, q_off=None, nk_arg=None, dh_arg=None):
    G, H, nq, nk, dh = c['G'], c['H'], c['nq'], c['nk'], c['dh']
    hd = H * dh
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], hd)          # [G, H, n, dh] -> [G, n, H * dh]
    al = c['align']
    q, qgs, qis = rows_buf(rows(d['q']), hd, 0 if c['q0'] else nq * hd + 8, off=(1 if al == 'ptr' else 0) if q_off is None else q_off)
    k, kgs, kis = rows_buf(rows(d['k']), hd + (1 if al == 'stride' else 4))
    v, vgs, vis = rows_buf(rows(d['v']), hd, nk * hd + 4)
    gamma = d['gamma'].reshape(-1).to(DEV)
    gate = ggs = gis = vres = rgs = ris = mix = mgs = mis = None
    if d['gate'] is not None:
        gate, ggs, gis = rows_buf(d['gate'].permute(0, 2, 1).contiguous(), H)
    if d['vres'] is not None:
        vres, rgs, ris = rows_buf(rows(d['vres']), hd + 8)
        mix, mgs, mis = rows_buf(d['mix'].permute(0, 2, 1).contiguous(), H + 3)
    lo, hi, last = restrict or c['restrict'] or (0, 0, 1)
    nq_out = hi - lo + last if hi > 0 else nq
    ois = hd
    ogs = nq_out * hd if c['ob'] else nq * hd + 4          # (the bf16 copy of the non-matrix-pipe forms needs contiguous output rows)
    out = Buf((G - 1) * ogs + nq_out * hd).upload()
    out_b = Buf(out.size, dtype=torch.bfloat16).upload() if c['ob'] else None
    P = lambda b: None if b is None else b.ptr
    Z = lambda s: 0 if s is None else s
    rc = lib.d4_small_attn(q.ptr, qgs, qis, k.ptr, kgs, kis, v.ptr, vgs, vis, P(gate), Z(ggs), Z(gis), _lib.ptr(gamma), P(vres), Z(rgs), Z(ris),
                           P(mix), Z(mgs), Z(mis), out.ptr, ogs, ois, P(out_b), G, H, nq, nk_arg or nk, c['clamp'], c['ms'], c['belief'], lo, hi, last,
                           dh_arg or dh, stream())
    torch.cuda.synchronize()
    return rc, out, out_b, (G, nq_out, hd, ogs, ois)


@pytest.mark.parametrize('c', K.SMALL_ATTN, ids=[c['name'] for c in K.SMALL_ATTN])
def test_small_attn(lib, c):
    d = K.small_attn_inputs(c)
    ref = K.small_attn_expect(c, d)                                                       # [G, H, nq_out, dh]
    rc, out, out_b, (G, nq_out, hd, ogs, ois) = small_attn_call(lib, c, d)
    _lib.check(rc)
    assert last_form(lib, 'small_attn') == c['form']
    want = Buf(out.size).host.double()
    want.as_strided((G, nq_out, hd), (ogs, ois, 1), GUARD).copy_(ref.permute(0, 2, 1, 3).reshape(G, nq_out, hd))
    note('small_attn', c['name'], check_image(out.dev, want, K.BOUND['small_attn']), K.BOUND['small_attn'])
    if out_b is not None:
        check_bf16_copy(out, out_b)


def _refused(lib, rc, out, frag):
    assert rc != 0
    assert frag in lib.d4_last_error().decode(), lib.d4_last_error().decode()
    assert out.dev.isnan().all(), 'a refused call wrote its output'


def test_small_attn_refuses_what_no_form_implements(lib):
    by = {c['name']: c for c in K.SMALL_ATTN}
    # the query restriction outside self attention over 8..16 tokens: the generic form, the small matrix-pipe forms, fewer than 8 tokens, the wide kernel
    for name in ('cross-16x17-dh32', 'cross-16x17-dh64-mis', 'cross-16x17-mfma', 'cross-7x7-mfma', 'cross-7x7-dh16', 'wide-self-65'):
        c = by[name]
        rc, out, _, _ = small_attn_call(lib, c, K.small_attn_inputs(c), restrict=(1, 4, 0))
        _refused(lib, rc, out, 'query restriction')
    c = by['wide-self-160']                                  # one key more than the wide kernel's limit (the operands hold 160: nothing is launched)
    rc, out, _, _ = small_attn_call(lib, c, K.small_attn_inputs(c), nk_arg=161)
    _refused(lib, rc, out, '161 keys (max 160)')
    c = by['cross-33x16-dh32']                               # a wide shape (65 keys) at head dim 32
    rc, out, _, _ = small_attn_call(lib, c, K.small_attn_inputs(c), nk_arg=65)
    _refused(lib, rc, out, 'head dim 32')
    c = by['wide-self-67']                                   # the wide kernel reads its query rows as float4
    rc, out, _, _ = small_attn_call(lib, c, K.small_attn_inputs(c), q_off=1)
    _refused(lib, rc, out, '16-byte aligned')


# ------------------------------------------------------------------------------------------------------------------- pool_mix
def pool_call(lib, c, d, *, L=None, D=None, heads=4):
    M, Lc, Dc = c['M'], c['L'], c['D']
    as16 = lambda t: t.to(torch.bfloat16).contiguous().to(DEV)
    q, k, hid, gw, gamma = (d[n].contiguous().to(DEV) for n in ('q', 'k', 'hid', 'gate_w', 'gamma'))
    x = None if c['x_last'] else d['x'].contiguous().to(DEV)
    xp = C.c_void_p(hid.data_ptr() + 4 * (Lc - 1) * M * Dc) if c['x_last'] else _lib.ptr(x)
    kb = as16(d['k']) if c['kb'] else None
    qb = as16(d['q']) if c['qb'] else None
    hb = as16(d['hid']) if c['hb'] else None
    u = Buf(M * 4 * Dc).upload()
    ub = Buf(M * 4 * Dc, dtype=torch.bfloat16).upload() if c['ub'] else None
    rc = lib.d4_pool_mix(None if c['qb'] else _lib.ptr(q), 256, xp, Dc, _lib.ptr(gw), None if c['kb'] else _lib.ptr(k), 256, _lib.ptr(hid), D or Dc,
                         _lib.ptr(gamma), u.ptr, M, L or Lc, heads, c['eps'], None if ub is None else ub.ptr, _lib.ptr(kb), _lib.ptr(qb), _lib.ptr(hb), stream())
    torch.cuda.synchronize()
    return rc, u, ub


@pytest.mark.parametrize('c', K.POOL_MIX, ids=[c['name'] for c in K.POOL_MIX])
def test_pool_mix(lib, c):
    d = K.pool_inputs(c)
    ref = K.pool_expect(c, d)                                                             # [M, 4, D]
    rc, u, ub = pool_call(lib, c, d)
    _lib.check(rc)
    assert last_form(lib, 'pool_mix') == c['form']
    want = Buf(u.size).host.double()
    want[GUARD:GUARD + u.size] = ref.reshape(-1)
    note('pool_mix', c['name'], check_image(u.dev, want, K.BOUND['pool_mix']), K.BOUND['pool_mix'])
    if ub is not None:
        check_bf16_copy(u, ub)


def test_pool_mix_refuses_what_it_does_not_cover(lib):
    c = next(c for c in K.POOL_MIX if c['name'] == 'pool-D1024-L64-M1-f32')
    d = K.pool_inputs(c)
    for kw, frag in ((dict(L=65), 'L=65'), (dict(D=1028), 'D=1028'), (dict(heads=3), '4 pool heads')):
        rc, u, _ = pool_call(lib, c, d, **kw)
        _refused(lib, rc, u, frag)


# ------------------------------------------------------------------------------------------------------------------- time decode
class TimeRun:
    """The device buffers of one time-decode case and the call."""

    def __init__(self, lib, c, d):
        self.lib, self.c = lib, c
        B, S, H, dh = c['B'], c['S'], c['H'], c['dh']
        self.hd, self.nc = H * dh, 3 * H * dh + 2 * H
        self.ldp = (self.nc + 3) // 4 * 4 + (1 if c['align'] == 'stride' else 4)
        self.poff = 1 if c['align'] == 'ptr' else 0
        self.gamma, self.inv = d['gamma'].reshape(-1).to(DEV), d['inv_freq'].to(DEV)
        self.cache = Buf(2 * c['cache_batch'] * c['cache_S'] * H * K.TCAP * dh).upload()

    def rows(self, proj, vres):
        B, Tq, S, _ = proj.shape
        p, _, _ = rows_buf(proj.reshape(1, B * Tq * S, self.nc), self.ldp, off=self.poff)
        return p, vres.reshape(-1).contiguous().to(DEV), B * Tq * S

    def call(self, mode, proj, vres, t0, cache, *, ob=False, t0_dev=None, Tcap=K.TCAP):
        c = self.c
        p, v, nrows = self.rows(proj, vres)
        o = Buf(nrows * self.hd).upload()
        o_b = Buf(nrows * self.hd, dtype=torch.bfloat16).upload() if ob else None
        tdev = None if t0_dev is None else torch.tensor([t0_dev], dtype=torch.int32, device=DEV)
        rc = self.lib.d4_time_attn_decode(p.ptr, self.ldp, _lib.ptr(v), self.hd, _lib.ptr(self.gamma), _lib.ptr(self.inv), cache.ptr, o.ptr, self.hd,
                                          None if o_b is None else o_b.ptr, c['B'], c['S'], c['H'], proj.shape[1], t0, Tcap, c['cache_batch'], c['cache_S'],
                                          _lib.ptr(tdev), c['clamp'], c['dh'], mode, stream())
        torch.cuda.synchronize()
        return rc, o, o_b


def _cache_image(cache, ref_cache):
    want = Buf(cache.size).host.double()
    want[GUARD:GUARD + cache.size] = ref_cache.reshape(-1)
    return want


def _out_image(out, ref_out):
    want = Buf(out.size).host.double()
    want[GUARD:GUARD + out.size] = ref_out.reshape(-1)
    return want


@pytest.mark.parametrize('c', K.TIME, ids=[c['name'] for c in K.TIME])
def test_time_decode(lib, c):
    d = K.time_inputs(c)
    ref_cache, ref_out = K.time_expect(c, d)
    bound = K.BOUND['time']
    r = TimeRun(lib, c, d)
    if c['kind'] == 'append':
        rc, o, _ = r.call(1, d['proj'], d['vres'], c['t0'], r.cache)
        _lib.check(rc)
        assert last_form(lib, 'time_kv_append') == c['kv_form']
        assert o.dev.isnan().all(), 'the append alone wrote the attention output'
        note('time', c['name'], check_image(r.cache.dev, _cache_image(r.cache, ref_cache), bound), bound)
        return
    pos = K.time_pos(c)
    if pos:                                                  # the history: one append of `pos` frames (checked with the final cache below)
        _lib.check(r.call(1, d['hist_proj'], d['hist_vres'], 0, r.cache)[0])
    cache_b = r.cache.clone()
    # A: the engine's call (append + attend)
    rc, out_a, out_ab = r.call(0, d['proj'], d['vres'], c['t0'], r.cache, ob=c['ob'], t0_dev=c['t0_dev'])
    _lib.check(rc)
    assert last_form(lib, 'time_attn') == c['attn_form0']
    if not c['fused']:
        assert last_form(lib, 'time_kv_append') == c['kv_form']
    # B: the two launchers one after the other
    _lib.check(r.call(1, d['proj'], d['vres'], c['t0'], cache_b, t0_dev=c['t0_dev'])[0])
    assert last_form(lib, 'time_kv_append') == c['kv_form']
    rc, out_b2, _ = r.call(2, d['proj'], d['vres'], c['t0'], cache_b, t0_dev=c['t0_dev'])
    _lib.check(rc)
    assert last_form(lib, 'time_attn') == c['attn_form']
    assert torch.equal(bits(out_a.dev), bits(out_b2.dev)), 'append + attend in one call and as two calls differ in the output bits'
    assert torch.equal(bits(r.cache.dev), bits(cache_b.dev)), 'append + attend in one call and as two calls leave different caches'
    e1 = check_image(r.cache.dev, _cache_image(r.cache, ref_cache), bound)
    e2 = check_image(out_a.dev, _out_image(out_a, ref_out), bound, scale=K.time_scale(c, ref_cache, ref_out))
    note('time', c['name'], max(e1, e2), bound)
    if out_ab is not None:
        check_bf16_copy(out_a, out_ab)


def test_time_decode_refuses_a_full_cache(lib):
    by = {c['name']: c for c in K.TIME}
    for name, mode, t0 in (('decode-H4-dh64-Tq1-t0-ok-cb', 0, K.TCAP), ('frames-H2-dh32-Tq5-t60-ok', 0, K.TCAP - 4), ('append-H3-dh64-Tq5-t0-ok-cb', 1, K.TCAP - 4),
                           ('frames-H4-dh64-Tq5-t60-ptr', 0, K.TCAP - 4)):
        c = by[name]
        d = K.time_inputs(c)
        r = TimeRun(lib, c, d)
        rc, o, _ = r.call(mode, d['proj'], d['vres'], t0, r.cache)
        assert rc != 0 and 'cache capacity 256 exceeded' in lib.d4_last_error().decode()
        assert r.cache.dev.isnan().all() and o.dev.isnan().all(), 'a refused call wrote the cache or the output'
    c = by['decode-H4-dh64-Tq1-t0-ok-cb']
    d = K.time_inputs(c)
    r = TimeRun(lib, c, d)
    rc, o, _ = r.call(3, d['proj'], d['vres'], 0, r.cache)
    assert rc != 0 and 'mode 3' in lib.d4_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------- coverage
def test_every_form_of_every_family_ran(lib):
    for fam, (err, name) in WORST.items():
        print(f'worst {fam}: {err:.3e} of bound {K.BOUND[fam]:.3e} ({name})')
    for fam, seen in SEEN.items():
        n = lib.d4_debug_forms(fam.encode(), 0, None)
        assert n > 0
        names = set()
        for i in range(n):
            s = C.c_char_p()
            assert lib.d4_debug_forms(fam.encode(), i, C.byref(s)) == n
            names.add(s.value.decode())
        assert len(names) == n
        assert seen == names, f'{fam}: never ran {sorted(names - seen)}; not in the list {sorted(seen - names)}'
    assert lib.d4_debug_forms(b'no_such_family', 0, None) == -1 and lib.d4_debug_last_form(b'no_such_family') is None
