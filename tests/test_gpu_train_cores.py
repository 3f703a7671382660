"""GPU: the attention cores of the training path (csrc/backward.hip: attn_bwd_kernel<DH,CAP>, xattn_bwd_kernel<DH>; csrc/attn_tiled.hip: the tiled
core in its time, within-frame and cross geometries) against the plain float64 reference of tests/train_core_ref.py, one core call per case
through d4_train_attn_core / d4_train_xattn_core: the cores the blocks call, without the RMSNorm, the GEMMs and the column sums around them.

A case (tests/train_core_cases.py) asserts
  * return code 0 and the form: d4_debug_last_form names the kernel the case was written for;
  * the values: every output within BOUND[family] of float64, per (group, head) problem (train_core_ref.problem_err);
  * ownership: outputs and the guards behind every buffer are pre-filled with one NaN bit pattern; after the call the owned region (q / k / v,
    gate and mix columns of dproj, o3, d_rv with residuals, dgamma_part; cross: q and gate columns of dprojq, k / v columns of dprojk) holds no
    NaN, and everything else (the pad columns between and behind the logit columns, the guards, d_rv without residuals, the guard behind the
    tiled core's planes) still holds that pattern; without residuals the mix column is +0.0 bit for bit; inputs are unchanged bit for bit;
  * the forward-only call (d_o3 null) gives the same o3 bit for bit and touches no gradient buffer;
  * once per form: a second call gives the same bits.
The core-0 and core-1 case of a shape run on the same inputs against the same reference (computed once on the CPU), and their difference is
recorded.  The refusals of the two entries return non-zero with a text that names the argument, before any launch.  The last test asserts that
the forms seen over the module are the library's full list for the families "train_attn" and "train_xattn" (d4_debug_forms): 13 + 6.

Tolerance (train_core_cases.py): E32 = float32 against float64 evaluation of the same reference on the CPU, worst case of the family,
recorded with 25 % headroom; the GPU bound is 8 x E32:
    family      measured E32   recorded E32   bound (8 x)
    self_lds    4.44e-6        5.6e-6         4.5e-5
    self_long   5.25e-6        6.6e-6         5.3e-5
    cross       1.00e-5        1.26e-5        1.0e-4"""
import ctypes as C

import pytest
import torch

import train_core_cases as K
import train_core_ref as R
from dreamer4_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAT = 0x7FC00D4A                 # the NaN every output, guard and plane is pre-filled with
SEEN = {'train_attn': set(), 'train_xattn': set()}
REPEATED = set()                 # forms whose second call was compared
WORST = {}                       # (family, tensor) -> (error / bound, case)
LDS_OUT = {}                     # key -> outputs of the core-0 case, for the comparison with core 1
CORE_DIFF = {}                   # tensor -> (largest |core 0 - core 1| / max |float64|, key)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def filled(n):
    return torch.full((n + K.GUARD,), PAT, dtype=torch.int32, device=DEV).view(torch.float32)


def loaded(x):
    if x is None:
        return None
    b = filled(x.numel())
    b[:x.numel()] = x.to(DEV)
    return b


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pat(t):
    return t.view(torch.int32) == PAT


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def last_form(lib, family):
    f = lib.d4_debug_last_form(family.encode())
    assert f is not None, f'no {family} form recorded'
    SEEN[family].add(f.decode())
    return f.decode()


def check_values(c, got, ref):
    errs = R.errors(got, ref)
    bound = K.BOUND[c['family']]
    for n, (e, et) in errs.items():
        print(f"{c['name']} {n}: err {e:.3e} per problem, {et:.3e} per tensor (bound {bound:.3e})")
        if e / bound > WORST.get((c['family'], n), (0., ''))[0]:
            WORST[(c['family'], n)] = (e / bound, c['name'])
    bad = {n: e for n, (e, _) in errs.items() if not e <= bound}
    assert not bad, f"{c['name']}: above the bound {bound:.3e}: {bad}"


def compare_cores(c, got, ref):
    if c['core'] == 0:
        LDS_OUT[c['key']] = got
    elif c['key'] in LDS_OUT:
        for n, a in LDS_OUT[c['key']].items():
            top = ref[n].abs().max().item() or ref['dv'].abs().max().item()
            d = (a.double() - got[n].double()).abs().max().item() / top
            if d >= CORE_DIFF.get(n, (-1., ''))[0]:
                CORE_DIFF[n] = (d, c['key'])


def owned_columns(ld, spans):
    m = torch.zeros(ld, dtype=torch.bool)
    for a, b in spans:
        m[a:b] = True
    return m


def check_owned(name, buf, rows, ld, cols):
    """buf: flat device buffer of rows x ld floats and the guard; cols: bool [ld], the columns the core owns in every row"""
    x = buf.cpu()
    body, guard = x[:rows * ld].view(rows, ld), x[rows * ld:]
    assert pat(guard).all(), f'{name}: the guard behind the buffer was written'
    assert not body[:, cols].isnan().any(), f'{name}: NaN in the owned region (a row or column was not written, or NaN was read)'
    assert pat(body[:, ~cols]).all(), f'{name}: {int((~pat(body[:, ~cols])).sum())} pad elements written'


# ------------------------------------------------------------------------------------------------------------------- self attention
class SelfCall:
    def __init__(self, lib, c):
        self.lib, self.c = lib, c
        self.rows, self.hd, self.ldp = K.self_rows_total(c), c['heads'] * c['dh'], K.self_ldp(c)
        self.d = K.inputs(c)
        self.inp = {k: loaded(v) for k, v in self.d.items()}
        self.pf = lib.d4_train_attn_core_plane_floats(self.rows, c['heads'], c['dh']) if c['core'] == 1 else 0

    def __call__(self, backward=True, **over):
        c, i = self.c, self.inp
        o = dict(o3=filled(self.rows * self.hd), dproj=filled(self.rows * self.ldp), d_rv=filled(self.rows * self.hd), dgamma=filled(c['groups'] * self.hd),
                 planes=filled(self.pf) if c['core'] == 1 else None)
        a = dict(proj=ptr(i['proj']), ldp=self.ldp, rv=ptr(i['rv']), gamma=ptr(i['gamma']), d_o3=ptr(i['d_o3']) if backward else None,
                 o3=ptr(o['o3']), dproj=ptr(o['dproj']), d_rv=ptr(o['d_rv']), dgamma=ptr(o['dgamma']), groups=c['groups'], items=c['items'],
                 heads=c['heads'], dh=c['dh'], clamp=c['clamp'], ns=c['ns'], belief=c['belief'], g_inner=c['g_inner'], outer=c['outer'], item=c['item'],
                 causal=int(c['geo'] == 'time'), inv_freq=ptr(i['inv_freq']), core=c['core'], planes=ptr(o['planes']), pf=self.pf)
        a.update(over)
        rc = self.lib.d4_train_attn_core(a['proj'], a['ldp'], a['rv'], a['gamma'], a['d_o3'], a['o3'], a['dproj'], a['d_rv'], a['dgamma'], a['groups'],
                                         a['items'], a['heads'], a['dh'], a['clamp'], a['ns'], a['belief'], a['g_inner'], a['outer'], a['item'],
                                         a['causal'], a['inv_freq'], a['core'], a['planes'], a['pf'], stream())
        torch.cuda.synchronize()
        return rc, o

    def gather(self, o):
        c, hd, H, dh = self.c, self.hd, self.c['heads'], self.c['dh']
        rows = R.self_rows(c['groups'], c['items'], c['g_inner'], c['outer'], c['item'])
        dp, n = o['dproj'].cpu()[:self.rows * self.ldp], self.rows * hd
        got = dict(o3=R.take(o['o3'].cpu()[:n], hd, rows, 0, H, dh), dq=R.take(dp, self.ldp, rows, 0, H, dh), dk=R.take(dp, self.ldp, rows, hd, H, dh),
                   dv=R.take(dp, self.ldp, rows, 2 * hd, H, dh), dgate=R.take(dp, self.ldp, rows, 3 * hd, H, 0),
                   dmix=R.take(dp, self.ldp, rows, 3 * hd + R.hp4_of(H), H, 0), dgamma_part=o['dgamma'].cpu()[:c['groups'] * hd].view(c['groups'], H, dh))
        if c['vres']:
            got['d_rv'] = R.take(o['d_rv'].cpu()[:n], hd, rows, 0, H, dh)
        return got

    def inputs_unchanged(self):
        for k, v in self.d.items():
            if v is not None:
                x = self.inp[k].cpu()
                assert same_bits(x[:v.numel()], v) and pat(x[v.numel():]).all(), f'input {k} changed'


@pytest.mark.parametrize('c', K.SELF, ids=[c['name'] for c in K.SELF])
def test_self_core(lib, c):
    call = SelfCall(lib, c)
    hd, H, rows = call.hd, c['heads'], call.rows
    rc, o = call()
    assert rc == 0, lib.d4_last_error().decode()
    assert last_form(lib, 'train_attn') == c['form']
    hp4 = R.hp4_of(H)
    check_owned('dproj', o['dproj'], rows, call.ldp, owned_columns(call.ldp, [(0, 3 * hd + H), (3 * hd + hp4, 3 * hd + hp4 + H)]))
    check_owned('o3', o['o3'], rows, hd, owned_columns(hd, [(0, hd)]))
    check_owned('d_rv', o['d_rv'], rows, hd, owned_columns(hd, [(0, hd)] if c['vres'] else []))
    check_owned('dgamma_part', o['dgamma'], c['groups'], hd, owned_columns(hd, [(0, hd)]))
    if o['planes'] is not None:
        assert pat(o['planes'][call.pf:]).all(), 'the guard behind the planes was written'
    if not c['vres']:
        mix = o['dproj'].cpu()[:rows * call.ldp].view(rows, call.ldp)[:, 3 * hd + hp4:3 * hd + hp4 + H]
        assert (mix.contiguous().view(torch.int32) == 0).all(), 'the mix-logit gradient without residuals is not +0.0'
    call.inputs_unchanged()
    ref = K.expect(c)
    got = call.gather(o)
    check_values(c, got, ref)
    compare_cores(c, got, ref)
    # forward only: the same o3, nothing else written
    rc, f = call(backward=False)
    assert rc == 0, lib.d4_last_error().decode()
    assert same_bits(f['o3'], o['o3']), 'the forward-only o3 differs from the o3 of the forward-and-backward call'
    for n in ('dproj', 'd_rv', 'dgamma'):
        assert pat(f[n]).all(), f'the forward-only call wrote {n}'
    if c['form'] not in REPEATED:
        REPEATED.add(c['form'])
        rc, o2 = call()
        assert rc == 0
        for n in ('o3', 'dproj', 'd_rv', 'dgamma'):
            assert same_bits(o[n], o2[n]), f'{n}: two calls differ'


# ------------------------------------------------------------------------------------------------------------------- cross attention
class CrossCall:
    def __init__(self, lib, c):
        self.lib, self.c = lib, c
        self.hd = c['heads'] * c['dh']
        self.ldq, self.ldk = K.cross_lds(c)
        self.rq, self.rk = c['groups'] * c['nq'], c['groups'] * c['nk']
        self.d = K.inputs(c)
        self.inp = {k: loaded(v) for k, v in self.d.items()}
        self.pf = lib.d4_train_xattn_core_plane_floats(self.rq, self.rk, c['heads'], c['dh']) if c['core'] == 1 else 0

    def __call__(self, backward=True, **over):
        c, i = self.c, self.inp
        o = dict(o3=filled(self.rq * self.hd), dprojq=filled(self.rq * self.ldq), dprojk=filled(self.rk * self.ldk), dgamma=filled(c['groups'] * self.hd),
                 planes=filled(self.pf) if c['core'] == 1 else None)
        a = dict(projq=ptr(i['projq']), ldq=self.ldq, projk=ptr(i['projk']), ldk=self.ldk, gamma=ptr(i['gamma']), d_o3=ptr(i['d_o3']) if backward else None,
                 o3=ptr(o['o3']), dprojq=ptr(o['dprojq']), dprojk=ptr(o['dprojk']), dgamma=ptr(o['dgamma']), groups=c['groups'], nq=c['nq'], nk=c['nk'],
                 heads=c['heads'], dh=c['dh'], item_major=c['item_major'], clamp=c['clamp'], core=c['core'], planes=ptr(o['planes']), pf=self.pf)
        a.update(over)
        rc = self.lib.d4_train_xattn_core(a['projq'], a['ldq'], a['projk'], a['ldk'], a['gamma'], a['d_o3'], a['o3'], a['dprojq'], a['dprojk'], a['dgamma'],
                                          a['groups'], a['nq'], a['nk'], a['heads'], a['dh'], a['item_major'], a['clamp'], a['core'], a['planes'], a['pf'],
                                          stream())
        torch.cuda.synchronize()
        return rc, o

    def gather(self, o):
        c, hd, H, dh = self.c, self.hd, self.c['heads'], self.c['dh']
        qrows, krows = R.cross_q_rows(c['groups'], c['nq']), R.cross_k_rows(c['groups'], c['nk'], c['item_major'])
        dq, dk = o['dprojq'].cpu()[:self.rq * self.ldq], o['dprojk'].cpu()[:self.rk * self.ldk]
        return dict(o3=R.take(o['o3'].cpu()[:self.rq * hd], hd, qrows, 0, H, dh), dq=R.take(dq, self.ldq, qrows, 0, H, dh),
                    dgate=R.take(dq, self.ldq, qrows, hd, H, 0), dk=R.take(dk, self.ldk, krows, 0, H, dh), dv=R.take(dk, self.ldk, krows, hd, H, dh),
                    dgamma_part=o['dgamma'].cpu()[:c['groups'] * hd].view(c['groups'], H, dh))

    def inputs_unchanged(self):
        for k, v in self.d.items():
            x = self.inp[k].cpu()
            assert same_bits(x[:v.numel()], v) and pat(x[v.numel():]).all(), f'input {k} changed'


@pytest.mark.parametrize('c', K.CROSS, ids=[c['name'] for c in K.CROSS])
def test_cross_core(lib, c):
    call = CrossCall(lib, c)
    hd, H = call.hd, c['heads']
    rc, o = call()
    assert rc == 0, lib.d4_last_error().decode()
    assert last_form(lib, 'train_xattn') == c['form']
    check_owned('dprojq', o['dprojq'], call.rq, call.ldq, owned_columns(call.ldq, [(0, hd + H)]))
    check_owned('dprojk', o['dprojk'], call.rk, call.ldk, owned_columns(call.ldk, [(0, 2 * hd)]))
    check_owned('o3', o['o3'], call.rq, hd, owned_columns(hd, [(0, hd)]))
    check_owned('dgamma_part', o['dgamma'], c['groups'], hd, owned_columns(hd, [(0, hd)]))
    if o['planes'] is not None:
        assert pat(o['planes'][call.pf:]).all(), 'the guard behind the planes was written'
    call.inputs_unchanged()
    ref = K.expect(c)
    got = call.gather(o)
    check_values(c, got, ref)
    compare_cores(c, got, ref)
    rc, f = call(backward=False)
    assert rc == 0, lib.d4_last_error().decode()
    assert same_bits(f['o3'], o['o3']), 'the forward-only o3 differs from the o3 of the forward-and-backward call'
    for n in ('dprojq', 'dprojk', 'dgamma'):
        assert pat(f[n]).all(), f'the forward-only call wrote {n}'
    if c['form'] not in REPEATED:
        REPEATED.add(c['form'])
        rc, o2 = call()
        assert rc == 0
        for n in ('o3', 'dprojq', 'dprojk', 'dgamma'):
            assert same_bits(o[n], o2[n]), f'{n}: two calls differ'


# ------------------------------------------------------------------------------------------------------------------- refusals
def _case(table, key, core):
    return next(c for c in table if c['key'] == key and c['core'] == core)


SELF_REFUSALS = [
    ('frame', 0, dict(proj=None), 'proj'), ('frame', 0, dict(gamma=None), 'gamma'), ('frame', 0, dict(o3=None), 'o3'),
    ('frame', 0, dict(dproj=None), 'dproj'), ('frame', 0, dict(dgamma=None), 'dgamma_part'), ('frame', 0, dict(d_rv=None), 'd_rv'),
    ('frame', 0, dict(dh=48), 'dim_head'), ('frame', 0, dict(items=0), 'items'), ('frame', 0, dict(items=65), 'items'),
    ('frame', 1, dict(items=1025), 'items'), ('frame', 0, dict(ldp='min-1'), 'ldp'), ('frame', 0, dict(causal=1), 'inv_freq'),
    ('time', 0, dict(causal=0), 'inv_freq'), ('frame', 0, dict(ns=-1), 'num_special'), ('frame', 0, dict(ns=33), 'num_special'),
    ('time', 0, dict(ns=1), 'num_special'), ('frame', 1, dict(planes=None), 'planes'), ('frame', 1, dict(pf='need-1'), 'plane_floats'),
    ('time', 1, dict(planes=None), 'planes'), ('frame', 0, dict(core=2), 'core 2'),
]


@pytest.mark.parametrize('geo,core,over,frag', SELF_REFUSALS, ids=[f'{g}-core{k}-{"-".join(o)}-{i}' for i, (g, k, o, _) in enumerate(SELF_REFUSALS)])
def test_self_core_refusals(lib, geo, core, over, frag):
    c = _case(K.SELF, {'frame': 'frame-dh32-n32', 'time': 'time-dh32-n16'}[geo], core)              # (both with residuals: d_rv is required)
    assert c['vres'] == 1
    call = SelfCall(lib, c)
    over = dict(over)
    if over.get('ldp') == 'min-1':
        over['ldp'] = 3 * call.hd + R.hp4_of(c['heads']) + c['heads'] - 1
    if over.get('pf') == 'need-1':
        over['pf'] = call.pf - 1
    rc, o = call(**over)
    assert rc != 0, f'{over} was accepted'
    assert frag in lib.d4_last_error().decode(), lib.d4_last_error().decode()
    for n in ('o3', 'dproj', 'd_rv', 'dgamma'):
        assert pat(o[n]).all(), f'a refused call wrote {n}'


CROSS_REFUSALS = [
    (0, dict(projq=None), 'projq'), (0, dict(projk=None), 'projk'), (0, dict(gamma=None), 'gamma'), (0, dict(o3=None), 'o3'),
    (0, dict(dprojq=None), 'dprojq'), (0, dict(dprojk=None), 'dprojk'), (0, dict(dgamma=None), 'dgamma_part'), (0, dict(dh=8), 'dim_head'),
    (0, dict(nq=0), 'nq'), (0, dict(nk=0), 'nk'), (0, dict(nq=65), 'nq'), (0, dict(nk=65), 'nk'), (1, dict(nq=1025), 'nq'), (1, dict(nk=1025), 'nk'),
    (0, dict(ldq='min-1'), 'ldq'), (0, dict(ldk='min-1'), 'ldk'), (1, dict(planes=None), 'planes'), (1, dict(pf='need-1'), 'plane_floats'),
    (0, dict(core=-1), 'core -1'),
]


@pytest.mark.parametrize('core,over,frag', CROSS_REFUSALS, ids=[f'core{k}-{"-".join(o)}-{i}' for i, (k, o, _) in enumerate(CROSS_REFUSALS)])
def test_cross_core_refusals(lib, core, over, frag):
    c = _case(K.CROSS, 'cross-3x20-dh32', core)
    call = CrossCall(lib, c)
    over = dict(over)
    if over.get('ldq') == 'min-1':
        over['ldq'] = call.hd + c['heads'] - 1
    if over.get('ldk') == 'min-1':
        over['ldk'] = 2 * call.hd - 1
    if over.get('pf') == 'need-1':
        over['pf'] = call.pf - 1
    rc, o = call(**over)
    assert rc != 0, f'{over} was accepted'
    assert frag in lib.d4_last_error().decode(), lib.d4_last_error().decode()
    for n in ('o3', 'dprojq', 'dprojk', 'dgamma'):
        assert pat(o[n]).all(), f'a refused call wrote {n}'


# ------------------------------------------------------------------------------------------------------------------- the forms
def test_every_form_of_the_two_families_was_seen(lib):
    total = 0
    for fam in SEEN:
        n = lib.d4_debug_forms(fam.encode(), 0, None)
        forms = set()
        for i in range(n):
            s = C.c_char_p()
            assert lib.d4_debug_forms(fam.encode(), i, C.byref(s)) == n
            forms.add(s.value.decode())
        assert len(forms) == n
        total += n
        assert SEEN[fam] == forms, f'{fam}: never launched {sorted(forms - SEEN[fam])}; not in the list {sorted(SEEN[fam] - forms)}'
        assert forms <= REPEATED
    assert total == 19
    for (fam, n), (e, name) in sorted(WORST.items()):
        print(f'largest error / bound: {fam} {n}: {e:.3f} ({name})')
    for n, (d, key) in sorted(CORE_DIFF.items()):
        print(f'largest core 0 - core 1 difference: {n}: {d:.3e} of max |float64| ({key})')
