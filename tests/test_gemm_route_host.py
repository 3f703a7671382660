"""CPU: the GEMM dispatcher's route (d4_gemm_route) against tests/golden/gemm_routes.npz, the answers of the routing predicates recorded with
tools/gemm_route_probe.cpp (its output, compressed) at the commit named in the golden's first line (before the route became one function).  Host logic only: the pointers are
fake and never dereferenced, nothing is launched, and without a device the CU count the persistent-kernel rule reads is 256, the MI355X's own.

Every cell of the golden is checked.  The grid holds SiLU-GLU calls (flags 5) with N % 64 != 0, which gemm() rejects whatever the predicates say: for
those cells the check is that d4_gemm_route returns -1 and names the reason; the equivalences below are asserted on every other cell."""
import ctypes as C
import os

import numpy as np
import pytest

from dreamer4_amd import _lib
from dreamer4_amd.build import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_routes.npz')
FLAGS = (0, 1, 2, 5, 8, 16, 24, 32)
KINDS = 5                              # 0 f32 only, 1 bf16 image, 2 bf16 image + Ab, 3 three planes, 4 two planes + scales
TILE, V2, V2_KSPLIT, X3, X3SK, H2, SKINNY, BF16, BF16A = range(9)      # include/d4hip.h: D4_GEMM_*
B_V2, B_X3SK, B_H2, B_SKINNY, B_KSPLIT = 1, 2, 4, 8, 16


@pytest.fixture(scope='module')
def lib():
    build()
    return _lib.load()


def desc(M, N, K, flags, kind, batch):
    """The call of one cell, as tools/gemm_route_probe.cpp builds it (its header has the list)."""
    d = _lib.GemmDesc()
    d.A, d.W, d.C, d.lda, d.ldw, d.ldc = 0x1000, 0x2000, 0x3000, K, K, N
    d.M, d.N, d.K, d.flags, d.rms_eps, d.batch = M, N, K, flags, 1e-6, batch
    if batch > 1:
        d.strideA, d.strideW, d.strideC = M * K, N * K, M * N
    if kind >= 1:
        d.Wb = 0x4000
    if kind == 2:
        d.Ab = 0x5000
    if kind >= 3:
        d.wplane = N * K * batch
    if kind == 4:
        d.wscale, d.strideWs = 0x6000, N
    return d


def tile_runs(c, flags):
    """csrc/gemm.hip, cfg_valid: which tiles of the first family have the SiLU-GLU epilogue (1, 3, 6) and the transposed-operand loads (0, 1, 3, 4)."""
    swiglu, trans = bool(flags & _lib.GEMM_SWIGLU), bool(flags & (_lib.GEMM_TRANS_A | _lib.GEMM_TRANS_B))
    return (c in (1, 3, 6) or not swiglu) and (c in (0, 1, 3, 4) or not trans)


def golden_lines():
    for line in np.load(GOLDEN)['text'].tobytes().decode().splitlines():     # the probe's output, byte for byte
        if line.startswith('#'):
            continue
        head, cells = line.split(':')
        M, N, K, batch, rule_M, rmap, forced = (int(x) for x in head.split())
        cells = cells.strip()
        assert len(cells) == 4 * len(FLAGS) * KINDS
        yield M, N, K, batch, rule_M, rmap, forced, cells


def test_route_matches_the_recorded_predicates(lib):
    checked = rejected = 0
    seen = set()
    try:
        for M, N, K, batch, rule_M, rmap, forced, cells in golden_lines():
            lib.d4_gemm_force_config(forced)
            for i, flags in enumerate(FLAGS):
                for kind in range(KINDS):
                    cell = cells[4 * (i * KINDS + kind):][:4]
                    bits, mask = int(cell[:2], 16), int(cell[2:], 16)
                    d = desc(M, N, K, flags, kind, batch)
                    fam = lib.d4_gemm_route(C.byref(d), rule_M)       # (the route does not read the row map: a family without it refuses at launch)
                    where = f'M{M} N{N} K{K} flags{flags} kind{kind} batch{batch} rule_M{rule_M} forced{forced}: family {fam}, recorded {cell}'
                    checked += 1
                    if flags & _lib.GEMM_SWIGLU and N % 64:
                        assert fam == -1 and 'swiglu needs N % 64' in lib.d4_last_error().decode(), where
                        rejected += 1
                        continue
                    assert 0 <= fam <= BF16A, where
                    seen.add(fam)
                    assert (fam == X3SK) == bool(bits & B_X3SK), where
                    if forced < 0:
                        assert (fam == V2) == bool(bits & B_V2), where
                    else:
                        assert not bits & B_V2, where                 # a forced call is not taken by rule
                    if kind == 4:
                        assert (fam == H2) == bool(bits & B_H2), where
                    else:
                        assert fam != H2 and not bits & B_H2, where
                    if kind == 0 and forced < 0:
                        assert (fam == SKINNY) == bool(bits & B_SKINNY), where
                        assert (fam == V2_KSPLIT) == (not bits & B_SKINNY and bool(bits & B_KSPLIT)), where
                    if kind == 0 and 0 <= forced < 8:
                        # gemm_config_valid(c, .) = "under force code c the call runs configuration c of the first family": the family is the first one
                        # (the few-row kernel comes first; no other family is reachable under such a code) AND the tile has the call's epilogue and
                        # layout — where it has not, the call stays in the family and the tuner picks.  So: bit c <=> TILE and the tile can run it, and
                        # TILE <=> any tile of the family can (configurations 1 and 3 run every call)
                        assert bool(mask >> forced & 1) == (fam == TILE and tile_runs(forced, flags)), where
                        assert (fam == TILE) == (mask != 0), where
                    if kind in (1, 2):
                        assert fam in (BF16, BF16A), where
    finally:
        lib.d4_gemm_force_config(-1)
    assert checked == 1800 * len(FLAGS) * KINDS and 0 < rejected < checked // 10
    assert seen == set(range(9)), seen                               # the grid reaches every family


def test_force_config_returns_the_family_counts(lib):
    """d4_gemm_force_config returns the number of configurations of the family it addressed (nothing forced: the first family's)."""
    try:
        got = {code: lib.d4_gemm_force_config(code) for code in (-1, 0, 100, 199, 200, 300, 400, 500)}
    finally:
        lib.d4_gemm_force_config(-1)
    fam = lib.d4_gemm_family_configs
    assert got == {-1: fam(TILE), 0: fam(TILE), 100: fam(V2), 199: fam(V2), 200: fam(BF16), 300: fam(X3), 400: fam(H2), 500: fam(BF16A)}
    assert got == {-1: 8, 0: 8, 100: 10, 199: 10, 200: 6, 300: 6, 400: 7, 500: 8}         # as recorded at the golden's commit


def test_route_rejects_what_gemm_rejects(lib):
    d = desc(640, 640, 64, 0, 0, 1)
    assert lib.d4_gemm_route(C.byref(d), 0) == V2
    d.lda = 66
    assert lib.d4_gemm_route(C.byref(d), 0) == -1 and 'multiples of 4' in lib.d4_last_error().decode()
    d = desc(640, 640, 64, _lib.GEMM_RMS_ROWSCALE | _lib.GEMM_TRANS_A, 0, 1)
    assert lib.d4_gemm_route(C.byref(d), 0) == -1 and 'rowscale' in lib.d4_last_error().decode()
