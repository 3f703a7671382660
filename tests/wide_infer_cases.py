"""Operator cases of the wide-frame inference attention core (csrc/attn_wide_mfma.hip: wide_attn_kernel<DH>, reached through
d4_small_attn_wide), shared by tests/test_gpu_wide_infer.py (the kernel against float64) and tests/test_wide_infer_host.py (the same
inputs on the CPU).  Cases have the shape of attn_core_cases._sa and use its input generator, its float64 reference and its tolerance
(E32 / BOUND of the 'small_attn' family: the host test asserts that the recorded E32 holds for these shapes too); seeds are this
table's own.

The shapes are the smallest at which the kernel can still go wrong: a wave owns 16 queries, a block 64, a key tile is 64 keys in four
16-key sub-tiles, so the sizes sit on both sides of 64 / 80 / 128 / 256, with one case at the cap of 1024 per side."""
import attn_core_cases as K

E32 = K.E32['small_attn']
BOUND = K.BOUND['small_attn']


def _form(dh):
    return f'wide_attn_kernel<{dh}>'


def _cases():
    cs = []
    # self attention with the belief projection: ragged last waves / blocks / key tiles, every head dim, value residual on and off
    for i, n in enumerate((65, 79, 80, 81, 128, 129, 257)):
        dh = (64, 32, 16)[i % 3]
        cs.append(K._sa(f'self-{n}-dh{dh}', _form(dh), n, n, dh, G=2, H=1 + i % 2, vres=i % 2, ms=(0, 1, 3)[i % 3], belief=1,
                        clamp=3. if i % 4 == 2 else 50., gate=int(i != 3), ob=int(i == 1)))
    cs.append(K._sa('self-1024-dh64', _form(64), 1024, 1024, 64, G=1, H=1, vres=1, ms=2, belief=1))
    # special blocks: alone in their own 16-key sub-tile, across a 64-key tile boundary, more than a tile of them, one, none
    cs.append(K._sa('special-80-ms16', _form(64), 80, 80, 64, G=2, H=2, vres=1, ms=16, belief=1))
    cs.append(K._sa('special-70-ms10', _form(32), 70, 70, 32, G=2, H=2, vres=0, ms=10, belief=1, clamp=3.))
    cs.append(K._sa('special-130-ms70', _form(16), 130, 130, 16, G=2, H=3, vres=1, ms=70, belief=1))
    cs.append(K._sa('special-97-ms1', _form(64), 97, 97, 64, G=2, H=1, vres=0, ms=1, belief=1))
    cs.append(K._sa('special-97-ms0', _form(32), 97, 97, 32, G=2, H=2, vres=1, ms=0, belief=1))
    # cross attention: one query over the cap, few and many queries with special keys, shared learned queries, both sides of 64
    cs.append(K._sa('cross-1x1023', _form(64), 1, 1023, 64, G=2, H=2))
    cs.append(K._sa('cross-1x1024', _form(16), 1, 1024, 16, G=2, H=2, vres=1))
    cs.append(K._sa('cross-5x200-ms3', _form(64), 5, 200, 64, G=2, H=2, ms=3, clamp=3.))
    cs.append(K._sa('cross-70x200-ms3', _form(32), 70, 200, 32, G=2, H=2, vres=1, ms=3))
    cs.append(K._sa('cross-300x16-q0', _form(64), 300, 16, 64, G=3, H=2, q0=1, ob=1))
    cs.append(K._sa('cross-16x300-dh32', _form(32), 16, 300, 32, G=2, H=3, gate=0))
    cs.append(K._sa('cross-65x64', _form(16), 65, 64, 16, G=2, H=2, vres=1))
    cs.append(K._sa('cross-64x65', _form(64), 64, 65, 64, G=2, H=1, clamp=3.))
    for k, c in enumerate(cs):
        c['seed'] = 5000 + k
    return cs


WIDE = _cases()

# the engine configurations of the oracle comparisons (keyword arguments of util.small_model on top of wide_frames=True)
ENGINE = dict(
    A=dict(num_spatial_tokens=70, num_latent_tokens=72, num_register_tokens=4, depth=4, time_block_every=2),
    B=dict(num_spatial_tokens=128, num_latent_tokens=6, num_register_tokens=0, depth=2, time_block_every=2, attn_dim_head=16, attn_heads=3, num_tasks=0),
    C=dict(num_spatial_tokens=60, num_latent_tokens=130, num_register_tokens=3, depth=3, time_block_every=1, attn_dim_head=32),
    D=dict(num_spatial_tokens=257, num_latent_tokens=257, num_register_tokens=0, depth=2, time_block_every=2, attn_heads=1),
)
