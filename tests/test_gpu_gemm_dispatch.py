"""GPU: the GEMM dispatcher end to end.  (a) The family d4_gemm_route names is the one that runs: with every profile class enabled the call counts one
launch, in a class of that family, with 2 M N K flops, and matches float64.  (b) The tuner per family, in fresh processes (its mode and table are read
once per process): a timed choice lands in the cache file under the family's id base, a strict run on that cache repeats the bits without timing, and a
strict run without the shape fails with the error that names the shipped table."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from dreamer4_amd import _lib
from test_gpu_kernels import run_gemm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, V2, V2_KSPLIT, SKINNY = 0, 1, 2, 6          # include/d4hip.h: D4_GEMM_*


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return _lib.load()


def route(lib, M, N, K, flags):
    """d4_gemm_route of the f32-only call run_gemm makes (host logic: the pointers only need their alignment)."""
    d = _lib.GemmDesc()
    d.A, d.W, d.C = 0x1000, 0x2000, 0x3000
    d.lda, d.ldw, d.ldc = K, N if flags & _lib.GEMM_TRANS_B else K, N
    d.M, d.N, d.K, d.flags, d.rms_eps, d.batch = M, N, K, flags, 1e-6, 1
    return lib.d4_gemm_route(C.byref(d), 0)


@pytest.mark.parametrize('M,N,K,tb,family', [(8, 256, 256, False, SKINNY), (128, 2048, 1024, False, V2_KSPLIT), (300, 520, 256, False, V2),
                                             (100, 200, 300, True, TILE)])
def test_the_routed_family_is_what_runs(lib, M, N, K, tb, family):
    assert route(lib, M, N, K, _lib.GEMM_TRANS_B if tb else 0) == family
    names = [lib.d4_profile_class_name(c).decode() for c in range(lib.d4_profile_classes())]
    of_family = {TILE: lambda n: n.startswith('gemm_kernel<'), V2: lambda n: n.startswith('gemm2_kernel<'), V2_KSPLIT: lambda n: n == 'gemm2_ksplit_kernel',
                 SKINNY: lambda n: False}[family]          # (the few-row kernel has no profile class)
    ms = (C.c_double * len(names))(); fl = (C.c_double * len(names))(); cnt = (C.c_int64 * len(names))()
    lib.d4_profile_enable((1 << len(names)) - 1)
    try:
        run_gemm(lib, M, N, K, tb=tb)                       # (asserts against float64)
        torch.cuda.synchronize()
        _lib.check(lib.d4_profile_read(ms, fl, cnt, len(names)))
    finally:
        lib.d4_profile_enable(0)
    ran = [c for c in range(len(names)) if cnt[c]]
    if family == SKINNY:
        assert ran == []
        return
    assert len(ran) == 1 and cnt[ran[0]] == 1, [(names[c], cnt[c]) for c in ran]
    assert of_family(names[ran[0]]), names[ran[0]]
    assert fl[ran[0]] == 2.0 * M * N * K


CHILD = r'''
import ctypes as C, sys, torch
from dreamer4_amd import _lib
lib = _lib.load()
out_dir, M = sys.argv[1], int(sys.argv[2])
g = torch.Generator(device='cuda').manual_seed(11)
A = torch.randn(M, 512, device='cuda', generator=g); W = torch.randn(512, 512, device='cuda', generator=g)
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for name, flags in (('tb', _lib.GEMM_TRANS_B), ('nt', 0)):
    o = torch.full((M, 512), float('nan'), device='cuda')
    rc = lib.d4_gemm(_lib.ptr(A), 512, _lib.ptr(W), 512, _lib.ptr(o), 512, None, None, 0, M, 512, 512, flags, 1e-6, s)
    torch.cuda.synchronize()
    print('RC', name, rc, lib.d4_last_error().decode() if rc else '')
    if rc == 0 and out_dir != '-':
        torch.save(o.cpu(), out_dir + '/' + name + '.' + sys.argv[3] + '.pt')
'''


def child(env, *args):
    full = {k: v for k, v in os.environ.items() if k not in ('D4_GEMM_TUNE_CACHE', 'D4_GEMM_AUTOTUNE')}
    full.update(env)
    r = subprocess.run([sys.executable, '-c', CHILD, *args], cwd=ROOT, env=full, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return {ln.split()[1]: (int(ln.split()[2]), ln.split(None, 3)[3] if len(ln.split()) > 3 else '') for ln in r.stdout.splitlines() if ln.startswith('RC ')}


def test_tuner_per_family_in_fresh_processes(lib, tmp_path):
    empty, cache = tmp_path / 'empty.txt', tmp_path / 'cache.txt'
    empty.write_text('')
    n2 = lib.d4_gemm_family_configs(V2)
    # 1: both calls (2 x 512^3 flops each, above the 1e8 threshold) are timed; the choices land in the cache under the families' id bases
    rcs = child({'D4_GEMM_TUNE_DEFAULT': str(empty), 'D4_GEMM_TUNE_CACHE': str(cache)}, str(tmp_path), '512', 'first')
    assert rcs == {'tb': (0, ''), 'nt': (0, '')}
    lines = [[int(x) for x in ln.split()] for ln in cache.read_text().splitlines()]
    assert len(lines) == 2 and all(ln[:3] == [512, 512, 512] and ln[4] == 1 for ln in lines), lines
    ids = {ln[3]: ln[5] for ln in lines}                    # flags -> id
    assert 0 <= ids[_lib.GEMM_TRANS_B] <= 7 and 100 <= ids[0] <= 100 + n2 - 1, lines
    # 2: strict mode on that cache times nothing, fails nothing, and repeats the bits
    rcs = child({'D4_GEMM_TUNE_DEFAULT': str(empty), 'D4_GEMM_TUNE_CACHE': str(cache), 'D4_GEMM_AUTOTUNE': 'strict'}, str(tmp_path), '512', 'second')
    assert rcs == {'tb': (0, ''), 'nt': (0, '')}
    assert len(cache.read_text().splitlines()) == 2
    for name in ('tb', 'nt'):
        assert torch.equal(torch.load(tmp_path / f'{name}.first.pt'), torch.load(tmp_path / f'{name}.second.pt'))
    # 3: strict mode, empty table, no cache, a shape of more than 512 rows: the host-side refusal (nothing is launched)
    rcs = child({'D4_GEMM_TUNE_DEFAULT': str(empty), 'D4_GEMM_AUTOTUNE': 'strict'}, '-', '1024', 'third')
    for name in ('tb', 'nt'):
        assert rcs[name][0] != 0 and 'gemm_tune_default.txt' in rcs[name][1] and 'M=1024 N=512 K=512' in rcs[name][1], rcs
