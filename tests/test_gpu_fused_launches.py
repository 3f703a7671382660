"""GPU: the launches only the engine reaches, one operator call per case through the C-ABI test entry points d4_gemm_run / d4_gemm_run_pair /
d4_tile16_weights / d4_frame_attn_out / d4_attn_out_cols / d4_frame_pool / d4_frame_pool_tail, each against a plain float64 reference.

GEMM epilogue options (every family, every configuration its `*_configs()` reports): the row-compacted second output C2 (bit for bit the row
gather of C, nothing else written) and GEMM_ACCUMULATE (float64 `epilogue + C0`), at the bound of the family's own accuracy test:
    fp32 families   2e-6 x max(1, |ref|max) x sqrt(max(1, K / 256))          (tests/test_gpu_kernels.py: run_gemm)
    bf16 families   3e-6 x ...  against float64 of the same rounded operands  (tests/test_gpu_bf16.py)
    x3, h2          3e-6 x ...                                                (their accuracy tests in tests/test_gpu_kernels.py)
A configuration is skipped only when the entry refuses the call with its "call not supported" error; the last GEMM test asserts that every
configuration of every family ran a C2 case and an ACCUMULATE case (the few-row / long-K form gemm2_ksplit implements neither: its refusal
is pinned instead).

Pairs: gemm_skinny_pair, gemm_bf16a_pair_launch, gemm2_pair_launch(c) against float64 and bit for bit against the two single launches.

Per-frame fused tails (tests/fused_cases.py, derivation of the bound there): each launch against float64 at BOUND[family] = 8 x E32, relative
to the output's max-abs; outputs, compact copies and every padding column pre-filled with NaN and checked untouched.
    family           measured E32   recorded E32   bound (8 x)
    frame_attn_out   2.13e-7        2.7e-7         2.2e-6
    attn_out_cols    1.58e-7        2.0e-7         1.6e-6
    frame_pool       5.02e-7        6.3e-7         5.0e-6      (frame_pool and frame_pool_tail)"""
import ctypes as C
import math

import pytest
import torch

import fused_cases as FC
import fused_ref as F
from dreamer4_amd import _lib
from test_gpu_attn_cores import DEV, GUARD, Buf, bits, check_image, stream

pytestmark = pytest.mark.gpu

EPS = 1.1920929e-07
RMS, SILU, SWIGLU, TA, TB, ACC = _lib.GEMM_RMS_ROWSCALE, _lib.GEMM_SILU, _lib.GEMM_SWIGLU, _lib.GEMM_TRANS_A, _lib.GEMM_TRANS_B, _lib.GEMM_ACCUMULATE
NAN = float('nan')
FAMILIES = {'tile': _lib.GEMM_TILE, 'v2': _lib.GEMM_V2, 'v2_ksplit': _lib.GEMM_V2_KSPLIT, 'x3': _lib.GEMM_X3, 'x3sk': _lib.GEMM_X3SK, 'h2': _lib.GEMM_H2,
            'skinny': _lib.GEMM_SKINNY, 'bf16': _lib.GEMM_BF16, 'bf16a': _lib.GEMM_BF16A}
FP32_BOUND = {'tile': 2e-6, 'v2': 2e-6, 'v2_ksplit': 2e-6, 'skinny': 2e-6, 'x3': 3e-6, 'x3sk': 3e-6, 'h2': 3e-6, 'bf16': 3e-6, 'bf16a': 3e-6}
# (smallest legal K, a K of 3 to 5 k-tiles) per family: the first family takes any K % 4 (a k tail behind its 32-wide tiles), the few-row kernel
# K % 4 in steps of 16, the LDS-DMA and split-operand families K % 32, the bf16-activation kernel K % 64
KS = {'tile': (8, 136), 'v2': (32, 128), 'v2_ksplit': (128, 160), 'x3': (32, 128), 'x3sk': (32, 128), 'h2': (32, 128), 'skinny': (4, 72), 'bf16': (32, 160),
      'bf16a': (64, 256)}
RAN = {}                         # (family, config) -> {'c2': runs, 'acc': runs, 'refused': refusals}
WORST = {}                       # family -> (error / bound, what)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def dptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def nan_f32(*shape):
    return torch.full(shape, NAN, device=DEV)


def nan_b16(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.bfloat16)


def tol(fam, ref, K):
    return FP32_BOUND[fam] * max(1., ref.abs().max().item()) * max(1., K / 256) ** 0.5


def note(fam, what, err, bound):
    if err / bound > WORST.get(fam, (0., ''))[0]:
        WORST[fam] = (err / bound, f'{what}: {err:.3e} of {bound:.3e}')


def n_configs(lib, fam):
    n = lib.d4_gemm_family_configs(FAMILIES[fam])
    assert n >= 1
    return n


# ------------------------------------------------------------------------------------------------------------------- GEMM operands
class Operands:
    """Seeded operands of one product in the form a family reads them, and the values the float64 reference is taken of."""

    def __init__(self, lib, fam, M, N, K, seed, lda=None, ta=False, tb=False):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.fam, self.M, self.N, self.K, self.ta, self.tb = fam, M, N, K, ta, tb
        Mp = (M + 3) // 4 * 4
        self.lda = lda or (Mp if ta else K)
        A_full = torch.randn((K, self.lda) if ta else (M, self.lda), device=DEV, generator=g)
        self.A_full = A_full
        A = A_full[:, :M] if ta else A_full[:, :K]
        W = torch.randn((K, N) if tb else (N, K), device=DEV, generator=g) / K ** 0.5
        self.W, self.ldw = W, W.shape[1]
        self.bias = torch.randn(N, device=DEV, generator=g)
        self.R = torch.randn(M, N, device=DEV, generator=g)
        self.C0 = torch.randn(M, N, device=DEV, generator=g)
        self.A_ref, self.W_ref, self.norm = A, W, None
        self.keep = []                                       # device tensors the descriptor points into
        d = self.base = dict(A=dptr(A_full), lda=self.lda, W=dptr(W), ldw=self.ldw)
        if fam in ('x3', 'x3sk'):
            n = W.numel()
            plane = (n + 7) // 8 * 8
            W3 = torch.zeros(3 * plane, dtype=torch.bfloat16, device=DEV)
            _lib.check(lib.d4_split_bf16x3(_lib.ptr(W), _lib.ptr(W3), n, plane, stream()))
            self.keep.append(W3)
            d.update(W=dptr(W3), Wb=dptr(W3), wplane=plane)
        elif fam == 'h2':
            plane = (N * K + 7) // 8 * 8
            W2 = torch.zeros(2 * plane, dtype=torch.float16, device=DEV)
            inv = torch.zeros(N, device=DEV)
            _lib.check(lib.d4_split_f16x2(_lib.ptr(W), _lib.ptr(W2), N, K, K, plane, _lib.ptr(inv), stream()))
            self.keep += [W2, inv]
            d.update(W=dptr(W2), Wb=dptr(W2), wplane=plane, wscale=dptr(inv))
        elif fam in ('bf16', 'bf16a'):
            Wb = W.to(torch.bfloat16).contiguous()
            self.keep.append(Wb)
            self.W_ref = Wb
            d.update(W=dptr(Wb), Wb=dptr(Wb))
            if fam == 'bf16':                                # fp32 activations rounded on the way in, the row scale from the unrounded ones
                self.A_ref, self.norm = A.to(torch.bfloat16), A
            else:
                Ab = A_full.to(torch.bfloat16).contiguous()
                self.keep.append(Ab)
                self.A_ref = Ab[:, :K]
                d.update(A=None, Ab=dptr(Ab))

    def ref(self, flags, bias=False, res=False, acc=False):
        return F.gemm_ref(self.A_ref, self.W_ref, flags=flags & 7, bias=self.bias if bias else None, R_=self.R if res else None,
                          C0=self.C0 if acc else None, eps=EPS, ta=self.ta, tb=self.tb, norm=self.norm)

    def desc(self, C_, ldc, flags, bias=False, res=False, **kw):
        d = _lib.GemmDesc()
        f = dict(self.base, C=dptr(C_), ldc=ldc, bias=dptr(self.bias) if bias else None, R=dptr(self.R) if res else None, ldr=self.N, M=self.M, N=self.N,
                 K=self.K, flags=flags, rms_eps=EPS, batch=1, c2_last=1)
        f.update(kw)
        for k, v in f.items():
            setattr(d, k, v.value if isinstance(v, C.c_void_p) else v)
        return d


def run(lib, fam, cfg, d, kind=None):
    """-> True when the call ran, False when the entry refused it as not supported (anything else is an error)."""
    rc = lib.d4_gemm_run(C.byref(d), FAMILIES[fam], cfg, stream())
    rec = RAN.setdefault((fam, cfg), {'c2': 0, 'acc': 0, 'refused': 0})
    if rc != 0:
        msg = lib.d4_last_error().decode()
        assert 'call not supported' in msg, msg
        rec['refused'] += 1
        return False
    torch.cuda.synchronize()
    if kind:
        rec[kind] += 1
    return True


BF16P = {'same': 0, 'diff': []}    # the phased kernel against configuration 0 on the same call: calls with equal bits, and the others


def bf16p_compare(what, phased, plain):
    """Recorded here, asserted by test_gemm_bf16p_bits_equal_a_plain_configuration: the other checks of a case do not depend on it."""
    bad = [(int((bits(a) != bits(b)).sum()), (a.double() - b.double()).abs().nan_to_num(0.).max().item()) for a, b in zip(phased, plain)
           if a is not None and not torch.equal(bits(a), bits(b))]
    if bad:
        BF16P['diff'].append(f'{what}: {sum(n for n, _ in bad)} elements differ, by at most {max(d for _, d in bad):.3e}')
    else:
        BF16P['same'] += 1


# ------------------------------------------------------------------------------------------------------------------- C2
C2_SHAPES = [(37, 15, 1, 5, 1), (37, 14, 1, 5, 0), (40, 11, 0, 11, 0), (40, 15, 3, 3, 1)]             # (frames, S, lo, hi, last); the last keeps only the last token
C2_SHAPES_SKINNY = [(1, 15, 1, 5, 1), (3, 15, 1, 5, 1), (25, 10, 1, 5, 0), (25, 10, 0, 10, 0), (3, 15, 3, 3, 1), (25, 10, 1, 5, 1)]      # M = 15, 45, 250


def c2_cases(fam):
    """-> (frames, S, lo, hi, last, N, ldc2, K)"""
    out = []
    for ki, K in enumerate(KS[fam]):
        for si, (fr, S, lo, hi, last) in enumerate(C2_SHAPES_SKINNY if fam == 'skinny' else C2_SHAPES):
            ns = [(320, 320)] if fr * S == 250 else [(320, 320), (300, 300)]
            if fam in ('v2', 'bf16a', 'tile') and (si + ki) % 2 == 0:
                ns += [(255, 255), (300, 304)]                                   # the scalar path, and a padded compact copy
            out += [(fr, S, lo, hi, last, N, ldc2, K) for N, ldc2 in ns]
    return out


def check_c2(fam, what, ops, C_, C2, Cb, C2b, case, ref):
    fr, S, lo, hi, last, N, ldc2, K = case
    M, keep = fr * S, hi - lo + last
    rows = torch.tensor([f * S + s for f in range(fr) for s in F.compact_rows(S, lo, hi, last)], device=DEV)
    assert C_[M:].isnan().all() and C2[fr * keep:].isnan().all() and C2[:, N:].isnan().all(), f'{what}: rows past the end or padding columns written'
    got = C_[:M]
    assert not got.isnan().any(), f'{what}: C not fully written'
    assert torch.equal(bits(C2[:fr * keep, :N]), bits(got[rows])), f'{what}: C2 is not the row gather of C'
    if Cb is not None:
        assert torch.equal(bits(Cb[:M]), bits(got.to(torch.bfloat16))), f'{what}: Cb is not the rounded C'
        assert C2b[fr * keep:].isnan().all() and C2b[:, N:].isnan().all()
        assert torch.equal(bits(C2b[:fr * keep, :N]), bits(Cb[:M][rows])), f'{what}: C2b is not the row gather of Cb'
    err, bound = (got.double() - ref).abs().max().item(), tol(fam, ref, K)
    note(fam, what, err, bound)
    assert err <= bound, f'{what}: err {err:.3e} > {bound:.3e}'


@pytest.mark.parametrize('fam', list(FAMILIES))
def test_gemm_compact_second_output(lib, fam):
    ncfg = n_configs(lib, fam)
    for ci, case in enumerate(c2_cases(fam)):
        fr, S, lo, hi, last, N, ldc2, K = case
        M, keep = fr * S, hi - lo + last
        ops = Operands(lib, fam, M, N, K, seed=100 + ci)
        flags, bias, res = ((0, False, True), (RMS, True, True), (SILU, True, False))[ci % 3]      # (the engine's call: no flags, residual)
        ref = ops.ref(flags, bias, res)
        plain = {}
        for cfg in range(ncfg):
            C_, C2 = nan_f32(M + 1, N), nan_f32(fr * keep + 2, ldc2)
            with_b = fam == 'bf16a'
            Cb, C2b = (nan_b16(M + 1, N), nan_b16(fr * keep + 2, ldc2)) if with_b else (None, None)
            d = ops.desc(C_, N, flags, bias, res, C2=dptr(C2), ldc2=ldc2, c2_S=S, c2_lo=lo, c2_hi=hi, c2_last=last, Cb=dptr(Cb), C2b=dptr(C2b))
            if not run(lib, fam, cfg, d, 'c2'):
                continue
            what = f'{fam}[{cfg}] C2 frames={fr} S={S} ({lo},{hi},{last}) N={N} ldc2={ldc2} K={K} flags={flags}'
            check_c2(fam, what, ops, C_, C2, Cb, C2b, case, ref)
            plain[cfg] = (C_, C2, Cb, C2b)
        if fam == 'bf16a' and 6 in plain and 0 in plain:     # the phased kernel: the same bits as a plain configuration, C2 included
            bf16p_compare(f'C2 case {case} flags={flags} bias={int(bias)} R={int(res)}', plain[6], plain[0])
        if fam == 'x3sk':                                    # the persistent form: the same bits as the plain 128 x 128 kernel
            C_, C2 = nan_f32(M + 1, N), nan_f32(fr * keep + 2, ldc2)
            d = ops.desc(C_, N, flags, bias, res, C2=dptr(C2), ldc2=ldc2, c2_S=S, c2_lo=lo, c2_hi=hi, c2_last=last)
            assert run(lib, 'x3', 4, d)
            assert torch.equal(bits(C_), bits(plain[0][0])) and torch.equal(bits(C2), bits(plain[0][1])), f'gemm_x3sk differs from gemm_x3 configuration 4 in case {case}'


# ------------------------------------------------------------------------------------------------------------------- ACCUMULATE
ACC_FLAGS = [(0, False, False), (RMS, False, False), (RMS, True, False), (SILU, True, True)]


def accumulate_case(lib, fam, ncfg, M, N, K, seed, flag_sets, ta=False, tb=False):
    ops = Operands(lib, fam, M, N, K, seed=seed, ta=ta, tb=tb)
    for flags, bias, res in flag_sets:
        ref = ops.ref(flags, bias, res, acc=True)
        f = flags | ACC | (TA if ta else 0) | (TB if tb else 0)
        outs = {}
        for cfg in range(ncfg):
            C_ = nan_f32(M + 1, N)
            C_[:M] = ops.C0
            with_b = fam == 'bf16a'
            Cb = nan_b16(M + 1, N) if with_b else None
            if not run(lib, fam, cfg, ops.desc(C_, N, f, bias, res, Cb=dptr(Cb)), 'acc'):
                continue
            what = f'{fam}[{cfg}] ACCUMULATE M={M} N={N} K={K} flags={f} bias={int(bias)} R={int(res)}'
            assert C_[M:].isnan().all(), f'{what}: a row past M written'
            err, bound = (C_[:M].double() - ref).abs().max().item(), tol(fam, ref, K)
            note(fam, what, err, bound)
            assert err <= bound, f'{what}: err {err:.3e} > {bound:.3e}'
            if with_b:
                assert torch.equal(bits(Cb[:M]), bits(C_[:M].to(torch.bfloat16))), f'{what}: Cb is not the rounded C'
            outs[cfg] = C_
        if fam == 'bf16a' and 6 in outs and 0 in outs:
            bf16p_compare(f'ACCUMULATE M={M} N={N} K={K} flags={f} bias={int(bias)} R={int(res)}', [outs[6]], [outs[0]])
        if fam == 'x3sk' and 0 in outs:
            C_ = nan_f32(M + 1, N)
            C_[:M] = ops.C0
            assert run(lib, 'x3', 4, ops.desc(C_, N, f, bias, res))
            assert torch.equal(bits(C_), bits(outs[0])), f'gemm_x3sk differs from gemm_x3 configuration 4 (ACCUMULATE, M={M} N={N} K={K} flags={f})'


@pytest.mark.parametrize('fam', list(FAMILIES))
def test_gemm_accumulate(lib, fam):
    ncfg = n_configs(lib, fam)
    kmin, kmul = KS[fam]
    # a partial-tile shape (the dispatcher gives the first family's 200 rows to the few-row kernel: its partial tiles are the 300 x 300 case), a full-tile one
    for i, (M, N, K) in enumerate([(200, 300, kmin), (300, 300, kmin), (256, 256, kmul), (512, 256, kmul)]):
        accumulate_case(lib, fam, ncfg, M, N, K, 300 + i, ACC_FLAGS)


def test_gemm_bf16p_bits_equal_a_plain_configuration():
    """The phased 256 x 256 kernel (csrc/gemm_bf16p.hip, configuration 6 of the bf16-activation family) against configuration 0 on every C2 and
    ACCUMULATE call above: the same bits in C, Cb, C2 and C2b.

    The row scale of the folded RMSNorm is where they could part: the phased kernel takes a row's sum of squares from the fragments it holds, and
    must form it in the plain kernels' order (one multiply-add chain per 16-byte chunk, the eight chunk sums as a balanced tree).  It summed in
    another order once, and every call with a row scale then differed in the last bit of a part of its outputs."""
    print(f'gemm_bf16p: {BF16P["same"]} calls bit-identical to configuration 0, {len(BF16P["diff"])} not')
    for line in BF16P['diff']:
        print('  ' + line)
    assert BF16P['same'] > 0, 'no call compared'
    assert not BF16P['diff'], f'{len(BF16P["diff"])} calls differ from configuration 0, e.g. ' + BF16P['diff'][0]


def test_gemm_accumulate_transposed_forms_of_the_backward(lib):
    """dX = dY W (TRANS_B) and dW = dY^T X (TRANS_A | TRANS_B) accumulate into their outputs (csrc/backward.hip, csrc/learn.hip): first family only."""
    ncfg = n_configs(lib, 'tile')
    for i, (M, N, K) in enumerate([(200, 300, 72), (256, 256, 128), (45, 388, 8)]):
        accumulate_case(lib, 'tile', ncfg, M, N, K, 400 + i, [(0, False, False), (0, True, True)], tb=True)
        accumulate_case(lib, 'tile', ncfg, M, N, K, 420 + i, [(0, False, False), (0, True, True)], ta=True, tb=True)


# ------------------------------------------------------------------------------------------------------------------- the few-row kernel alone
@pytest.mark.parametrize('K', [64, 512, 1040, 1376, 1536, 2048])
def test_gemm_skinny_row_groups_and_instances(lib, K):
    """gemm_skinny.hip: one, two and sixteen 16-row groups with a partial last one; K covers the four (waves, load steps) instances and both edges
    of the six-step one (K in 1040 .. 1536)."""
    for mi, M in enumerate((1, 16, 17, 33, 250)):
        N = 320 if M == 250 else (388, 64, 255, 1024, 320)[mi]
        ops = Operands(lib, 'skinny', M, N, K, seed=500 + mi)
        for flags, bias, res in ((0, False, False), (RMS, True, False), (SILU, True, True)):
            C_ = nan_f32(M + 1, N)
            assert run(lib, 'skinny', 0, ops.desc(C_, N, flags, bias, res))
            ref = ops.ref(flags, bias, res)
            assert C_[M:].isnan().all()
            err, bound = (C_[:M].double() - ref).abs().max().item(), tol('skinny', ref, K)
            note('skinny', f'skinny M={M} N={N} K={K} flags={flags}', err, bound)
            assert err <= bound, f'skinny M={M} N={N} K={K} flags={flags}: err {err:.3e} > {bound:.3e}'
    if K in (1376, 2048):                                    # SiLU-GLU on packed column pairs
        for M, N in ((17, 192), (33, 128)):
            ops = Operands(lib, 'skinny', M, N, K, seed=520 + M)
            C_ = nan_f32(M + 1, N // 2)
            assert run(lib, 'skinny', 0, ops.desc(C_, N // 2, RMS | SWIGLU, True, False))
            ref = ops.ref(RMS | SWIGLU, True, False)
            assert C_[M:].isnan().all()
            err, bound = (C_[:M].double() - ref).abs().max().item(), tol('skinny', ref, K)
            note('skinny', f'skinny SiLU-GLU M={M} N={N} K={K}', err, bound)
            assert err <= bound
    # strided batch of 3
    M, N, B = 17, 72, 3
    g = torch.Generator(device=DEV).manual_seed(540 + K)
    A = torch.randn(B, M + 1, K, device=DEV, generator=g); W = torch.randn(B, N + 2, K, device=DEV, generator=g) / K ** 0.5
    R = torch.randn(B, M + 3, N, device=DEV, generator=g); bias = torch.randn(N, device=DEV, generator=g)
    C_ = nan_f32(B, M + 3, N)
    d = _lib.GemmDesc()
    for k, v in dict(A=A.data_ptr(), lda=K, W=W.data_ptr(), ldw=K, C=C_.data_ptr(), ldc=N, bias=bias.data_ptr(), R=R.data_ptr(), ldr=N, M=M, N=N, K=K, flags=SILU,
                     rms_eps=EPS, batch=B, strideA=(M + 1) * K, strideW=(N + 2) * K, strideC=(M + 3) * N, c2_last=1).items():
        setattr(d, k, v)
    assert run(lib, 'skinny', 0, d)
    assert C_[:, M:].isnan().all()
    for b in range(B):
        ref = F.gemm_ref(A[b, :M], W[b, :N], flags=SILU, bias=bias, R_=R[b, :M], eps=EPS)
        assert (C_[b, :M].double() - ref).abs().max().item() <= tol('skinny', ref, K)


def test_every_configuration_of_every_family_ran_both_options(lib):
    for fam, (frac, what) in sorted(WORST.items()):
        print(f'worst {fam}: {frac:.2f} of its bound ({what})')
    for fam in FAMILIES:
        ncfg = n_configs(lib, fam)
        ran = [c for c in range(ncfg) if RAN.get((fam, c), {}).get('c2', 0) and RAN[(fam, c)]['acc']]
        print(f'{fam}: {ncfg} configurations; C2 runs {[RAN.get((fam, c), {}).get("c2", 0) for c in range(ncfg)]}, ACCUMULATE runs '
              f'{[RAN.get((fam, c), {}).get("acc", 0) for c in range(ncfg)]}, refusals {[RAN.get((fam, c), {}).get("refused", 0) for c in range(ncfg)]}')
        if fam == 'v2_ksplit':                               # implements neither option: gemm2_ksplit_applicable refuses both, every time
            assert RAN[(fam, 0)]['c2'] == 0 and RAN[(fam, 0)]['acc'] == 0 and RAN[(fam, 0)]['refused'] > 0
        else:
            assert ran == list(range(ncfg)), f'{fam}: configurations {sorted(set(range(ncfg)) - set(ran))} never ran a C2 case and an ACCUMULATE case'
    assert lib.d4_gemm_family_configs(99) == -1


# ------------------------------------------------------------------------------------------------------------------- pairs
def pair_run(lib, a, b, target, cfg=0):
    rc = lib.d4_gemm_run_pair(C.byref(a), C.byref(b), target, cfg, stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('K', [64, 512, 1376, 2048])
def test_gemm_skinny_pair(lib, K):
    """The engine's lopsided pair: a query projection of a few rows (lda = S x D) beside a key projection; one side with bias + R, the other with C2."""
    for si, ((M1, N1, lda1), (M2, N2), (S, lo, hi, last)) in enumerate([((1, 520, 15 * K), (15, 1024), (15, 1, 5, 1)), ((16, 260, K), (250, 128), (10, 1, 5, 0)),
                                                                        ((33, 64, K), (5, 2064), (5, 1, 4, 1))]):
        for flags in (RMS, 0):
            oa = Operands(lib, 'skinny', M1, N1, K, seed=600 + si, lda=lda1)
            ob = Operands(lib, 'skinny', M2, N2, K, seed=620 + si)
            fr, keep = M2 // S, hi - lo + last
            c2kw = lambda C2: dict(C2=dptr(C2), ldc2=N2, c2_S=S, c2_lo=lo, c2_hi=hi, c2_last=last)
            Ca, Cb_, C2 = nan_f32(M1 + 1, N1), nan_f32(M2 + 1, N2), nan_f32(fr * keep + 1, N2)
            rc = pair_run(lib, oa.desc(Ca, N1, flags, True, True), ob.desc(Cb_, N2, flags, **c2kw(C2)), _lib.PAIR_SKINNY)
            _lib.check(rc)
            Ra, Rb, R2 = nan_f32(M1 + 1, N1), nan_f32(M2 + 1, N2), nan_f32(fr * keep + 1, N2)
            assert run(lib, 'skinny', 0, oa.desc(Ra, N1, flags, True, True)) and run(lib, 'skinny', 0, ob.desc(Rb, N2, flags, **c2kw(R2)))
            what = f'skinny pair ({M1},{N1},{lda1}) + ({M2},{N2}) K={K} flags={flags}'
            assert torch.equal(bits(Ca), bits(Ra)) and torch.equal(bits(Cb_), bits(Rb)) and torch.equal(bits(C2), bits(R2)), f'{what}: differs from two gemm_skinny calls'
            check_c2('skinny', what, ob, Cb_, C2, None, None, (fr, S, lo, hi, last, N2, N2, K), ob.ref(flags))
            ref = oa.ref(flags, True, True)
            assert Ca[M1:].isnan().all()
            err, bound = (Ca[:M1].double() - ref).abs().max().item(), tol('skinny', ref, K)
            note('skinny', what, err, bound)
            assert err <= bound, f'{what}: err {err:.3e} > {bound:.3e}'


@pytest.mark.parametrize('Mbig,tile', [(1216, 2), (2432, 1)])       # gemm_bf16a_rule: 64 x 64 tiles at 1216 x 1024, 128 x 64 at 2432 x 1024
@pytest.mark.parametrize('K', [64, 192])
def test_gemm_bf16a_pair(lib, K, Mbig, tile):
    """gemm_bf16a_pair_launch in both tiles it supports: the pool's key projection (many rows) with the query projection (few rows, strided lda)
    riding in its grid; once with fp32 + bf16 outputs on both sides, once with the key side's bf16 image alone (C == nullptr)."""
    for si, Msmall in enumerate((5, 130)):
        big = Operands(lib, 'bf16a', Mbig, 1024, K, seed=700 + si)
        small = Operands(lib, 'bf16a', Msmall, 520, K, seed=720 + si, lda=3 * K + 8)
        for only_b in (False, True):
            def outs():
                return (None if only_b else nan_f32(Mbig + 1, 1024)), nan_b16(Mbig + 1, 1024), nan_f32(Msmall + 1, 520), nan_b16(Msmall + 1, 520)
            C1, B1, C2_, B2 = outs()
            da, db = big.desc(C1, 1024, RMS, Cb=dptr(B1)), small.desc(C2_, 520, RMS, Cb=dptr(B2))
            _lib.check(pair_run(lib, da, db, _lib.PAIR_BF16A))
            R1, RB1, R2, RB2 = outs()
            assert run(lib, 'bf16a', tile, big.desc(R1, 1024, RMS, Cb=dptr(RB1))) and run(lib, 'bf16a', tile, small.desc(R2, 520, RMS, Cb=dptr(RB2)))
            what = f'bf16a pair {Mbig}x1024 + {Msmall}x520 K={K} only_b={only_b}'
            for got, want in ((C1, R1), (B1, RB1), (C2_, R2), (B2, RB2)):
                if got is not None:
                    assert torch.equal(bits(got), bits(want)), f'{what}: differs from two gemm_bf16a_launch calls of tile {tile}'
            for ops, Cf, Cb, M in ((big, C1, B1, Mbig), (small, C2_, B2, Msmall)):
                ref = ops.ref(RMS)
                assert Cb[M:].isnan().all() and not Cb[:M].isnan().any()
                if Cf is not None:
                    assert Cf[M:].isnan().all()
                    err, bound = (Cf[:M].double() - ref).abs().max().item(), tol('bf16a', ref, K)
                    note('bf16a', what, err, bound)
                    assert err <= bound, f'{what}: err {err:.3e} > {bound:.3e}'
                    assert torch.equal(bits(Cb[:M]), bits(Cf[:M].to(torch.bfloat16)))
                else:                                        # the image alone: on top of the bound one rounding to bf16's 8 significant bits, at most
                    over = (Cb[:M].double() - ref).abs() - 2. ** -8 * ref.abs()      # half an ulp = 2^-8 of an element just above a power of two
                    assert over.max().item() <= tol('bf16a', ref, K), f'{what}: bf16-only output off by {over.max().item():.3e} beyond its rounding'


def test_gemm_bf16a_pair_refusals_stay_refusals(lib):
    K = 64
    big, small = Operands(lib, 'bf16a', 1216, 1024, K, seed=740), Operands(lib, 'bf16a', 5, 520, K, seed=741)
    other_k = Operands(lib, 'bf16a', 5, 520, 128, seed=742)
    C1, C2_ = nan_f32(1216, 1024), nan_f32(5, 520)
    cc = nan_f32(8, 520)
    ok = lambda: small.desc(C2_, 520, RMS)
    for what, db in (('unequal K', other_k.desc(C2_, 520, RMS)), ('a bias', small.desc(C2_, 520, RMS, True)), ('a residual', small.desc(C2_, 520, RMS, False, True)),
                     ('a C2', small.desc(C2_, 520, RMS, C2=dptr(cc), ldc2=520, c2_S=5, c2_lo=1, c2_hi=3, c2_last=1)), ('flags 0', small.desc(C2_, 520, 0)),
                     ('flags RMS | SiLU', small.desc(C2_, 520, RMS | SILU))):
        rc = pair_run(lib, big.desc(C1, 1024, RMS), db, _lib.PAIR_BF16A)
        assert rc != 0 and 'call not supported' in lib.d4_last_error().decode(), what
        assert C1.isnan().all() and C2_.isnan().all() and cc.isnan().all(), f'{what}: a refused pair wrote an output'
    _lib.check(pair_run(lib, big.desc(C1, 1024, RMS), ok(), _lib.PAIR_BF16A))


def test_gemm2_pair_every_pair_configuration(lib):
    """gemm2_pair_launch(c) for every configuration gemm2_pair_config_ok admits, on the smallest shape of test_gemm_pair_is_bit_identical_to_two_launches."""
    M1, M2, N1, N2, K = 40, 5000, 256, 256, 512
    oa, ob = Operands(lib, 'v2', M1, N1, K, seed=800), Operands(lib, 'v2', M2, N2, K, seed=801)
    ra, rb = oa.ref(RMS), ob.ref(RMS)
    ran = []
    for cfg in range(n_configs(lib, 'v2')):
        C1, C2_ = nan_f32(M1 + 1, N1), nan_f32(M2 + 1, N2)
        rc = pair_run(lib, oa.desc(C1, N1, RMS), ob.desc(C2_, N2, RMS), _lib.PAIR_V2, cfg)
        if rc != 0:
            assert 'call not supported' in lib.d4_last_error().decode() and C1.isnan().all() and C2_.isnan().all()
            continue
        ran.append(cfg)
        R1, R2 = nan_f32(M1 + 1, N1), nan_f32(M2 + 1, N2)
        assert run(lib, 'v2', cfg, oa.desc(R1, N1, RMS)) and run(lib, 'v2', cfg, ob.desc(R2, N2, RMS))
        assert torch.equal(bits(C1), bits(R1)) and torch.equal(bits(C2_), bits(R2)), f'gemm2 pair configuration {cfg} differs from two launches'
        for Cf, ref, M in ((C1, ra, M1), (C2_, rb, M2)):
            err, bound = (Cf[:M].double() - ref).abs().max().item(), tol('v2', ref, K)
            note('v2', f'gemm2 pair cfg {cfg}', err, bound)
            assert err <= bound
    assert ran == [0, 2, 4, 6, 8, 9], ran                    # V2_64x64, 128x64_8, 128x64_k16, 32x64, 32x32, 64x32 (gemm2_pair_config_ok)


# ------------------------------------------------------------------------------------------------------------------- tile16_weights
@pytest.mark.parametrize('N,K,ldw', [(16, 4, 4), (512, 512, 516), (272, 512, 512)])
def test_tile16_weights_is_the_index_permutation(lib, N, K, ldw):
    W = torch.randn(N, ldw, generator=torch.Generator().manual_seed(N + K))
    src = Buf(N * ldw)
    src.view((N, ldw), (ldw, 1)).copy_(W)
    src.upload()
    dst = Buf(N * K).upload()
    _lib.check(lib.d4_tile16_weights(src.ptr, ldw, dst.ptr, N, K, stream()))
    torch.cuda.synchronize()
    want = Buf(N * K).host.clone()
    want[GUARD:GUARD + N * K] = F.tile16_ref(W, N, K).reshape(-1)
    got = dst.dev.cpu()
    assert torch.equal(bits(got[GUARD:GUARD + N * K]), bits(want[GUARD:GUARD + N * K])) and got[:GUARD].isnan().all() and got[GUARD + N * K:].isnan().all()


def test_tile16_weights_refusals(lib):
    src, dst = Buf(512 * 516).upload(), Buf(512 * 512).upload()
    for N, K, ldw in ((24, 512, 512), (32, 6, 8), (32, 512, 514)):
        rc = lib.d4_tile16_weights(src.ptr, ldw, dst.ptr, N, K, stream())
        torch.cuda.synchronize()
        assert rc != 0 and 'tile16_weights' in lib.d4_last_error().decode()
        assert dst.dev.isnan().all()


# ------------------------------------------------------------------------------------------------------------------- frame_attn_out / attn_out_cols
LDP = 3 * FC.HD + 2 * FC.H + 8                               # a row of the fused projection: q | k | v | gate logits | mix logits (+ a gap)
LDV = FC.HD + 8


class AttnFrame:
    """Device operands of one within-frame attention tail, laid out as the engine's fused projection lays them out."""

    def __init__(self, c, d):
        Fr, S, D, hd, H = c['frames'], c['S'], c['D'], FC.HD, FC.H
        rows = lambda t: t.permute(0, 2, 1, 3).reshape(Fr * S, hd)               # [F, H, S, dh] -> [F * S, H * dh]
        self.proj = Buf(Fr * S * LDP)
        pv = self.proj.view((Fr * S, LDP), (LDP, 1))
        pv[:, 0:hd], pv[:, hd:2 * hd], pv[:, 2 * hd:3 * hd] = rows(d['q']), rows(d['k']), rows(d['v'])
        pv[:, 3 * hd:3 * hd + H] = d['gate'].permute(0, 2, 1).reshape(Fr * S, H)
        self.vres = None
        if d['vres'] is not None:
            pv[:, 3 * hd + H:3 * hd + 2 * H] = d['mix'].permute(0, 2, 1).reshape(Fr * S, H)
            self.vres = Buf(Fr * S * LDV)
            self.vres.view((Fr * S, LDV), (LDV, 1))[:, :hd] = rows(d['vres'])
            self.vres.upload()
        self.proj.upload()
        self.gamma = d['gamma'].reshape(-1).to(DEV)
        self.ld = D + c['pad']
        self.resid = Buf(Fr * S * self.ld)
        self.resid.view((Fr * S, D), (self.ld, 1)).copy_(d['resid'].reshape(Fr * S, D))
        self.resid.upload()
        self.c, self.c2 = c, FC._c2(c)
        self.keep = FC.keep_rows(c)

    def outputs(self):
        c = self.c
        out = Buf(c['frames'] * c['S'] * self.ld).upload()
        c2 = Buf(c['frames'] * self.keep * self.ld).upload() if self.c2 else None
        return out, c2

    def attn_args(self, frames=None, S=None, heads=FC.H, q_off=0, out_b=None):
        c, hd, H, S_ = self.c, FC.HD, FC.H, self.c['S']
        p = lambda off: C.c_void_p(self.proj.ptr.value + 4 * off)
        gs = S_ * LDP
        v = self.vres
        return [p(q_off), gs, LDP, p(hd), gs, LDP, p(2 * hd), gs, LDP, p(3 * hd), gs, LDP, _lib.ptr(self.gamma),
                None if v is None else v.ptr, 0 if v is None else S_ * LDV, 0 if v is None else LDV, None if v is None else p(3 * hd + H), 0 if v is None else gs,
                0 if v is None else LDP, out_b, frames or c['frames'], heads, S or S_, c['clamp'], c['ms'], c['belief'], 64]

    def tail_args(self, out, c2, ldr=None):
        lo, hi, last = self.c2 or (0, 0, 0)
        return [self.resid.ptr, ldr or self.ld, out.ptr, self.ld, None if c2 is None else c2.ptr, self.ld, lo, hi, last, stream()]

    def images(self, out, c2, ref):
        """The float64 images the two outputs must equal, NaN in the padding columns."""
        c, D = self.c, self.c['D']
        w1 = Buf(out.size).host.double()
        w1.as_strided((c['frames'] * c['S'], D), (self.ld, 1), GUARD).copy_(ref[0].reshape(-1, D))
        w2 = None
        if c2 is not None:
            w2 = Buf(c2.size).host.double()
            w2.as_strided((c['frames'] * self.keep, D), (self.ld, 1), GUARD).copy_(ref[1].reshape(-1, D))
        return w1, w2


def check_tail(family, name, out, c2, images):
    bound = FC.BOUND[family]
    err = check_image(out.dev, images[0], bound)
    if c2 is not None:
        err = max(err, check_image(c2.dev, images[1], bound))
    print(f'{family} {name}: err {err:.3e} (bound {bound:.3e})')
    note(family, name, err, bound)


@pytest.mark.parametrize('c', FC.FRAME_ATTN_OUT, ids=[c['name'] for c in FC.FRAME_ATTN_OUT])
def test_frame_attn_out(lib, c):
    d = FC.attn_inputs(c)
    ref = FC.attn_expect(c, d)
    fr = AttnFrame(c, d)
    wo_t = F.tile16_ref(d['Wo'], c['D'], FC.HD).reshape(-1).to(DEV)
    out, c2 = fr.outputs()
    _lib.check(lib.d4_frame_attn_out(*fr.attn_args(), _lib.ptr(wo_t), c['D'], *fr.tail_args(out, c2)))
    torch.cuda.synchronize()
    check_tail('frame_attn_out', c['name'], out, c2, fr.images(out, c2, ref))


def _small_attn_then_gemm(lib, fr, c, d):
    """attn_mfma_kernel<1,1> into a dense [frames * S][512] buffer, then the few-row GEMM with the residual and the compact copy."""
    Fr, S, D, hd, H = c['frames'], c['S'], c['D'], FC.HD, FC.H
    a = fr.attn_args()
    att = Buf(Fr * S * hd).upload()
    _lib.check(lib.d4_small_attn(*a[:19], att.ptr, S * hd, hd, None, Fr, H, S, S, c['clamp'], c['ms'], c['belief'], 0, 0, 1, 64, stream()))
    torch.cuda.synchronize()
    assert lib.d4_debug_last_form(b'small_attn') == b'attn_mfma_kernel<1,1>'
    out, c2 = fr.outputs()
    lo, hi, last = fr.c2 or (0, 0, 1)
    g = _lib.GemmDesc()
    for k, v in dict(A=att.ptr.value, lda=hd, W=fr.W.ptr.value, ldw=c['ldw'], C=out.ptr.value, ldc=fr.ld, R=fr.resid.ptr.value, ldr=fr.ld, M=Fr * S, N=D, K=hd, flags=0,
                     rms_eps=EPS, batch=1, C2=None if c2 is None else c2.ptr.value, ldc2=fr.ld, c2_S=S, c2_lo=lo, c2_hi=hi, c2_last=last).items():
        setattr(g, k, v)
    _lib.check(lib.d4_gemm_run(C.byref(g), _lib.GEMM_SKINNY, 0, stream()))
    torch.cuda.synchronize()
    return out, c2


def _cols_weights(c, d):
    W = Buf(c['D'] * c['ldw'])
    W.view((c['D'], FC.HD), (c['ldw'], 1)).copy_(d['Wo'])
    return W.upload()


@pytest.mark.parametrize('c', FC.ATTN_OUT_COLS, ids=[c['name'] for c in FC.ATTN_OUT_COLS])
def test_attn_out_cols(lib, c):
    d = FC.attn_inputs(c)
    ref = FC.attn_expect(c, d)
    fr = AttnFrame(c, d)
    fr.W = _cols_weights(c, d)
    out, c2 = fr.outputs()
    _lib.check(lib.d4_attn_out_cols(*fr.attn_args(), fr.W.ptr, c['ldw'], c['D'], *fr.tail_args(out, c2)))
    torch.cuda.synchronize()
    check_tail('attn_out_cols', c['name'], out, c2, fr.images(out, c2, ref))
    # the kernel's promise: the bits of attn_mfma_kernel followed by the few-row GEMM with the residual
    out2, c22 = _small_attn_then_gemm(lib, fr, c, d)
    assert torch.equal(bits(out.dev), bits(out2.dev)), 'attn_out_cols differs from small_attn + the few-row GEMM'
    if c2 is not None:
        assert torch.equal(bits(c2.dev), bits(c22.dev)), 'attn_out_cols: the compact copy differs from small_attn + the few-row GEMM'


def _refused(lib, rc, frag, *bufs):
    assert rc != 0
    assert frag in lib.d4_last_error().decode(), lib.d4_last_error().decode()
    for b in bufs:
        assert b is None or b.dev.isnan().all(), 'a refused call wrote an output'


def test_attn_out_cols_refusals(lib):
    c = next(c for c in FC.ATTN_OUT_COLS if c['name'].startswith('aoc-G4-S11-D512'))
    d = FC.attn_inputs(c)
    fr = AttnFrame(c, d)
    fr.W = _cols_weights(c, d)
    out, c2 = fr.outputs()
    ob = Buf(out.size, dtype=torch.bfloat16).upload()
    w_mis = C.c_void_p(fr.W.ptr.value + 4)
    for kw, W in ((dict(frames=5), fr.W.ptr), (dict(out_b=ob.ptr), fr.W.ptr), (dict(), w_mis)):
        rc = lib.d4_attn_out_cols(*fr.attn_args(**kw), W, c['ldw'], c['D'], *fr.tail_args(out, c2))
        torch.cuda.synchronize()
        _refused(lib, rc, 'attn_out_cols: call not supported', out, c2, ob)


def test_frame_attn_out_refusals_are_host_side(lib):
    """Frame counts outside 192 .. 1024, more than 16 tokens, another head count, a bf16 image asked for (the kernel has none to write and the
    engine never asks: its bf16 mode does not take this path), a leading dimension or a query pointer that breaks the float4 accesses."""
    c = next(c for c in FC.FRAME_ATTN_OUT if c['name'].startswith('fao-F192-S15-D512-v1'))
    d = FC.attn_inputs(c)
    fr = AttnFrame(c, d)
    wo_t = F.tile16_ref(d['Wo'], c['D'], FC.HD).reshape(-1).to(DEV)
    out, c2 = fr.outputs()
    ob = Buf(out.size, dtype=torch.bfloat16).upload()
    for kw, ldr in ((dict(frames=191), None), (dict(frames=1025), None), (dict(S=17), None), (dict(heads=7), None), (dict(out_b=ob.ptr), None),
                    (dict(), c['D'] + 2), (dict(q_off=1), None)):
        rc = lib.d4_frame_attn_out(*fr.attn_args(**kw), _lib.ptr(wo_t), c['D'], *fr.tail_args(out, c2, ldr=ldr))
        torch.cuda.synchronize()
        _refused(lib, rc, 'frame_attn_out: call not supported', out, c2, ob)


# ------------------------------------------------------------------------------------------------------------------- frame_pool / frame_pool_tail
class PoolFrame:
    def __init__(self, c, d):
        M, L, D = c['M'], c['L'], c['D']
        up = lambda t: t.contiguous().to(DEV)
        self.q, self.k, self.hid, self.gw, self.gamma = up(d['q']), up(d['k']), up(d['hid']), up(d['gate_w']), up(d['gamma'])
        self.x = None if c['x_last'] else up(d['x'])
        self.xp = C.c_void_p(self.hid.data_ptr() + 4 * (L - 1) * M * D) if c['x_last'] else _lib.ptr(self.x)
        self.wv_t = F.tile16_ref(d['Wv'], FC.HP, D).reshape(-1).to(DEV)
        self.wo_t = F.tile16_ref(d['Wo'], D, FC.HP).reshape(-1).to(DEV)
        self.c, self.c2, self.keep, self.ld = c, FC._c2(c), FC.keep_rows(c), D + c['pad']
        self.resid = Buf(M * self.ld)
        self.resid.view((M, D), (self.ld, 1)).copy_(d['resid'].reshape(M, D))
        self.resid.upload()

    outputs = AttnFrame.outputs
    images = AttnFrame.images

    def tail_args(self, out, c2, ldr=None):
        lo, hi, last = self.c2 or (0, 0, 0)
        return [self.resid.ptr, ldr or self.ld, out.ptr, self.ld, None if c2 is None else c2.ptr, self.ld, lo, hi, last, stream()]

    def pool(self, lib, out, c2, frames=None, S=None, heads=4, ldr=None, q_off=0):
        c = self.c
        return lib.d4_frame_pool(C.c_void_p(self.q.data_ptr() + 4 * q_off), 256, self.xp, c['D'], _lib.ptr(self.gw), _lib.ptr(self.k), 256, _lib.ptr(self.hid), c['D'],
                                 _lib.ptr(self.gamma), c['M'], c['L'], heads, c['eps'], _lib.ptr(self.wv_t), _lib.ptr(self.wo_t), frames or c['frames'], S or c['S'],
                                 *self.tail_args(out, c2, ldr))

    def tail(self, lib, u, out, c2, frames=None, S=None, heads=4, ldr=None):
        c = self.c
        return lib.d4_frame_pool_tail(_lib.ptr(u), _lib.ptr(self.wv_t), _lib.ptr(self.wo_t), frames or c['frames'], S or c['S'], c['D'], heads,
                                      *self.tail_args(out, c2, ldr))


@pytest.mark.parametrize('c', FC.FRAME_POOL, ids=[c['name'] for c in FC.FRAME_POOL])
def test_frame_pool_and_tail(lib, c):
    d = FC.pool_inputs(c)
    ref = FC.pool_expect(c, d)
    pf = PoolFrame(c, d)
    out, c2 = pf.outputs()
    _lib.check(pf.pool(lib, out, c2))
    torch.cuda.synchronize()
    check_tail('frame_pool', c['name'], out, c2, pf.images(out, c2, ref))
    # the tail alone, from the mixes of the stand-alone pool_mix kernel
    u = nan_f32(c['M'], 4, c['D'])
    _lib.check(lib.d4_pool_mix(_lib.ptr(pf.q), 256, pf.xp, c['D'], _lib.ptr(pf.gw), _lib.ptr(pf.k), 256, _lib.ptr(pf.hid), c['D'], _lib.ptr(pf.gamma), _lib.ptr(u),
                               c['M'], c['L'], 4, c['eps'], None, None, None, None, stream()))
    out, c2 = pf.outputs()
    _lib.check(pf.tail(lib, u, out, c2))
    torch.cuda.synchronize()
    check_tail('frame_pool', c['name'] + '-tail', out, c2, pf.images(out, c2, ref))


def test_frame_pool_refusals_are_host_side(lib):
    c = next(c for c in FC.FRAME_POOL if c['name'].startswith('pool-F192-S11-L5'))
    d = FC.pool_inputs(c)
    pf = PoolFrame(c, d)
    out, c2 = pf.outputs()
    u = nan_f32(c['M'], 4, c['D'])
    for kw in (dict(frames=191), dict(frames=1025), dict(S=17), dict(heads=3), dict(ldr=c['D'] + 2)):
        for which, call in (('frame_pool', lambda: pf.pool(lib, out, c2, **kw)), ('frame_pool_tail', lambda: pf.tail(lib, u, out, c2, **kw))):
            rc = call()
            torch.cuda.synchronize()
            _refused(lib, rc, f'{which}: call not supported', out, c2)
    rc = pf.pool(lib, out, c2, q_off=1)                      # the mix reads its query rows as float4
    torch.cuda.synchronize()
    _refused(lib, rc, 'd4_frame_pool: operand missing / not 16-byte aligned', out, c2)


def test_worst_errors_of_the_fused_tails():
    for fam in ('frame_attn_out', 'attn_out_cols', 'frame_pool'):
        frac, what = WORST.get(fam, (0., 'no case ran'))
        print(f'worst {fam}: {frac:.2f} of its bound ({what})')
        assert fam in WORST
