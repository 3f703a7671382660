"""Host: the workspaces of the space and cross attention blocks with and without d4_train_wide_set (the size queries launch nothing), and
the condition that keeps the bounds of tests/test_gpu_wide_frames.py from hiding anything: the oracle evaluated in float32 stays within a
tenth of those bounds of its float64 evaluation at every new operator shape."""
import pytest
import torch

from dreamer4_amd import _lib
from wide_frames_cases import CROSS_WIDE, SPACE_WIDE, cross_oracle, cross_oracle_run, space_oracle, space_oracle_run

FRAMES, DIM, DIMC, HEADS, DH, GROUPS = 3, 64, 32, 2, 64, 3
PART = 8 << 20                                                     # DW_PART_FLOATS
r64 = lambda n: (n + 63) // 64 * 64


def space_ws(tokens):
    return _lib.load().d4_attn_workspace_bytes(FRAMES, tokens, DIM, HEADS, DH)


def cross_ws(nq, nk):
    return _lib.load().d4_cross_attn_workspace_bytes(GROUPS, nq, nk, DIM, DIMC, HEADS, DH)


def lds_space_ws(tokens):
    """csrc/backward.hip attn_ws without the planes of the tiled core: every array rounded up to 64 floats."""
    R, hd = FRAMES * tokens, HEADS * DH
    hp4 = (HEADS + 3) // 4 * 4
    P = (3 * hd + 2 * hp4 + 31) // 32 * 32
    arrays = [R * DIM, P * DIM, P, R * P, R * P, R * hd, R * hd, P * DIM, R * DIM, R * DIM, FRAMES * hd, PART, P * DIM]
    return 4 * sum(r64(n) for n in arrays)


def lds_cross_ws(nq, nk):
    """csrc/backward.hip x_ws without the planes of the tiled core."""
    Rq, Rk, hd = GROUPS * nq, GROUPS * nk, HEADS * DH
    hp4 = (HEADS + 3) // 4 * 4
    Pq, Pk = hd + hp4, 2 * hd
    arrays = [Rq * DIM, Rk * DIMC, Pq * DIM, Pk * DIMC, Rq * Pq, Rk * Pk, Rq * Pq, Rk * Pk, Rq * hd, Rq * hd, Pq * DIM, Pk * DIMC,
              Rq * DIM, Rq * DIM, Rk * DIMC, Rk * DIMC, GROUPS * hd, PART, max(Pk, Pq) * max(DIM, DIMC)]
    return 4 * sum(r64(n) for n in arrays)


@pytest.fixture
def wide_on():
    lib = _lib.load()
    assert lib.d4_train_wide_set(1) == 0
    try:
        yield
    finally:
        assert lib.d4_train_wide_set(0) == 1


def test_switch_off_the_workspaces_are_the_lds_cores():
    for tokens in (16, 64, 70, 256):
        assert space_ws(tokens) == lds_space_ws(tokens), tokens
    for nq, nk in ((1, 7), (64, 64), (4, 256)):
        assert cross_ws(nq, nk) == lds_cross_ws(nq, nk), (nq, nk)


def test_switch_on_the_workspaces_change_above_64_only(wide_on):
    for tokens in (16, 64):
        assert space_ws(tokens) == lds_space_ws(tokens), tokens
    for tokens in (65, 70, 256):
        assert space_ws(tokens) > lds_space_ws(tokens), tokens
    for nq, nk in ((1, 7), (64, 64)):
        assert cross_ws(nq, nk) == lds_cross_ws(nq, nk), (nq, nk)
    for nq, nk in ((4, 256), (65, 3), (1, 65)):
        assert cross_ws(nq, nk) > lds_cross_ws(nq, nk), (nq, nk)


def test_switch_on_the_workspaces_grow_linearly(wide_on):
    d = lambda n: space_ws(2 * n) - space_ws(n)
    assert 0 < d(512) <= 2.05 * d(256)
    d = lambda n: cross_ws(4, 2 * n) - cross_ws(4, n)
    assert 0 < d(512) <= 2.05 * d(256)


def test_the_switch_returns_the_previous_state():
    lib = _lib.load()
    try:
        assert lib.d4_train_wide_set(1) == 0
        assert lib.d4_train_wide_set(1) == 1
        assert lib.d4_train_wide_set(5) == 1                      # any non-zero value is "on"
    finally:
        assert lib.d4_train_wide_set(0) == 1
    assert lib.d4_train_wide_set(0) == 0
    assert space_ws(70) == lds_space_ws(70)


def worst(f32, f64):
    """Largest difference of any tensor, relative to the tensor's scale as test_gpu_backward.close measures it."""
    assert set(f32) == set(f64)
    w = 0.
    for k in f64:
        scale = max(f64[k].abs().max().item(), 1e-6)
        w = max(w, (f32[k].double() - f64[k]).abs().max().item() / scale)
    return w


@pytest.mark.parametrize('shape', SPACE_WIDE)
def test_fp32_oracle_is_within_a_tenth_of_the_gpu_bound_space(shape):
    w = worst(space_oracle_run(shape, torch.float32), space_oracle(shape))
    print(f'\nspace {shape}: fp32 vs float64 oracle, worst tensor {w:.2e} of scale')
    assert w <= 2e-5


@pytest.mark.parametrize('shape', CROSS_WIDE)
def test_fp32_oracle_is_within_a_tenth_of_the_gpu_bound_cross(shape):
    w = worst(cross_oracle_run(shape, torch.float32), cross_oracle(shape))
    print(f'\ncross {shape}: fp32 vs float64 oracle, worst tensor {w:.2e} of scale')
    assert w <= 2e-5
