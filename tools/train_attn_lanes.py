"""Lane-level CPU emulation of the fragment algebra of csrc/attn_tiled_bf16.hip against plain matrix products, on exact integer
data: the score-type products from the row-major images (head dims 64, 32, 16 with its zero-padded contraction), the accumulator pair as the
A operand in the slot order 8 kq + j <-> item 16 (j >> 2) + 4 kq + (j & 3), the B operand from the transposed images, in both orientations
(fwd / dq: S^T tiles, keys on the accumulator rows; dkv: S tiles, queries on the rows).  No GPU; prints one line per check and exits non-zero
on a mismatch.

The emulated instruction, v_mfma_f32_16x16x32_bf16:  D[m][n] = C[m][n] + sum_k A[m][k] B[k][n]  with
    A element j of lane l: m = l & 15, k = 8 (l >> 4) + j;   B element j of lane l: n = l & 15, k = 8 (l >> 4) + j;
    C / D register r of lane l: m = 4 (l >> 4) + r, n = l & 15."""
import sys

import numpy as np


def mfma(a, b, c):
    """a, b [64][8], c [64][4] (per lane) -> d [64][4]"""
    A, B = np.zeros((16, 32), np.int64), np.zeros((32, 16), np.int64)
    for l in range(64):
        for j in range(8):
            A[l & 15, 8 * (l >> 4) + j] = a[l, j]
            B[8 * (l >> 4) + j, l & 15] = b[l, j]
    D = A @ B
    d = c.copy()
    for l in range(64):
        for r in range(4):
            d[l, r] += D[4 * (l >> 4) + r, l & 15]
    return d


def load_frag(img, row0, n, dh):
    """load_frag of the kernel for the 64 lanes: row row0 + tok of a row-major image [n][dh] -> list of KS fragments [64][8]"""
    ks = 2 if dh == 64 else 1
    out = [np.zeros((64, 8), np.int64) for _ in range(ks)]
    for l in range(64):
        tok, kq = l & 15, l >> 4
        row = row0 + tok
        if row < n and (dh > 16 or kq < 2):
            c0 = 8 * kq if dh > 16 else 8 * (kq & 1)
            for s in range(ks):
                out[s][l] = img[row, c0 + 32 * s:c0 + 32 * s + 8]
    return out


def dot_frag(a, b):
    c = np.zeros((64, 4), np.int64)
    for fa, fb in zip(a, b):
        c = mfma(fa, fb, c)
    return c


def pack_pair(lo, hi):
    return np.concatenate([lo, hi], axis=1)


def acc_items(acc, a, timg, r0, dh):
    """acc[t] += A B over items r0 .. r0 + 31 of the transposed image [dh][np]"""
    for t in range(dh // 16):
        b = np.zeros((64, 8), np.int64)
        for l in range(64):
            tok, kq = l & 15, l >> 4
            src = timg[16 * t + tok]
            b[l, :4] = src[r0 + 4 * kq:r0 + 4 * kq + 4]
            b[l, 4:] = src[r0 + 16 + 4 * kq:r0 + 16 + 4 * kq + 4]
        acc[t] = mfma(a, b, acc[t])


def tile_rows(c):
    """accumulator [64][4] -> matrix [16 rows][16 columns]"""
    m = np.zeros((16, 16), np.int64)
    for l in range(64):
        for r in range(4):
            m[4 * (l >> 4) + r, l & 15] = c[l, r]
    return m


def check(dh, n_own, n_walk, rng):
    """One wave: 16 `own` rows (fwd / dq: queries; dkv: keys) against all `walk` items, 32 per step, as the kernels do: the score tile has
    the walked items on its rows, is used as the A operand of the accumulate-type product, and the result has the own rows on its rows."""
    own = rng.integers(-3, 4, (n_own, dh))
    walk = rng.integers(-3, 4, (n_walk, dh))
    payload = rng.integers(-3, 4, (n_walk, dh))                        # the rows the second product sums (v, k', q or dO)
    npad = (n_walk + 31) // 32 * 32
    timg = np.zeros((dh, npad), np.int64)
    timg[:, :n_walk] = payload.T
    fo = load_frag(own, 0, n_own, dh)
    acc = [np.zeros((64, 4), np.int64) for _ in range(dh // 16)]
    scores = np.zeros((npad, 16), np.int64)
    for r0 in range(0, n_walk, 32):
        st = []
        for u in range(2):
            if r0 + 16 * u >= n_walk:
                st.append(np.zeros((64, 4), np.int64))
                continue
            st.append(dot_frag(load_frag(walk, r0 + 16 * u, n_walk, dh), fo))     # rows: walked items, columns: own rows
            scores[r0 + 16 * u:r0 + 16 * u + 16] = tile_rows(st[u])
        acc_items(acc, pack_pair(st[0], st[1]), timg, r0, dh)
    s_ref = np.zeros((npad, 16), np.int64)
    s_ref[:n_walk, :min(n_own, 16)] = walk @ own[:16].T
    out_ref = s_ref[:n_walk].T @ payload                               # [16 own rows][dh]
    out = np.concatenate([tile_rows(a) for a in acc], axis=1)
    return np.array_equal(scores, s_ref) and np.array_equal(out, out_ref)


def main():
    rng = np.random.default_rng(0)
    bad = 0
    for dh in (64, 32, 16):
        for n_own, n_walk in ((16, 32), (16, 64), (5, 17), (16, 33), (1, 1), (16, 100)):
            ok = check(dh, n_own, n_walk, rng)
            print(f'dh {dh:2d}  own rows {n_own:2d}  walked items {n_walk:3d}: {"exact" if ok else "MISMATCH"}')
            bad += not ok
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
