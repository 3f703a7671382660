"""Host: the workspace of the training time-attention block — unchanged at <= 64 frames, linear in the frames above (the tiled core,
csrc/attn_tiled.hip, adds per-row planes only; nothing of size frames x frames)."""
from dreamer4_amd import _lib

DIM, HEADS, DH, BATCH, TOKENS = 64, 2, 64, 1, 2


def ws(frames):
    return _lib.load().d4_time_attn_workspace_bytes(BATCH, frames, TOKENS, DIM, HEADS, DH)


def lds_core_ws(frames):
    """csrc/backward.hip attn_ws as it stood before the tiled core: every array rounded up to 64 floats."""
    R, F, hd = BATCH * frames * TOKENS, BATCH * TOKENS, HEADS * DH
    hp4 = (HEADS + 3) // 4 * 4
    P = (3 * hd + 2 * hp4 + 31) // 32 * 32
    arrays = [R * DIM, P * DIM, P, R * P, R * P, R * hd, R * hd, P * DIM, R * DIM, R * DIM, F * hd, 8 << 20, P * DIM]
    return 4 * sum((n + 63) // 64 * 64 for n in arrays)


def test_workspace_is_unchanged_up_to_64_frames():
    assert ws(64) == lds_core_ws(64)
    assert ws(16) == lds_core_ws(16)


def test_workspace_grows_linearly_above_64_frames():
    d = lambda f: ws(2 * f) - ws(f)
    assert ws(65) > lds_core_ws(65)                      # the planes of the tiled core are there
    assert 0 < d(512) <= 2.05 * d(256)
