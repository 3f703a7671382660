"""Operator cases of the chunked AttentionPool mix (csrc/pool_mix_deep.hip, reached through d4_pool_mix_deep) and the engine
configurations of the deep-trunk tests, shared by tests/test_gpu_deep_pool.py (the kernel against float64) and
tests/test_deep_pool_host.py (the same inputs on the CPU).  Cases have the shape of attn_core_cases._pm and use its input generator and
its float64 reference; seeds are this table's own.

The tolerance is the family's own: E32 is the largest error of the float32 evaluation of attn_core_ref.pool_mix_ref against its float64
evaluation over THIS table (a softmax over up to 1024 hiddens sums more terms than one over 64), measured on the CPU and recorded with a
quarter of headroom; the GPU bound is 8 x E32 (attn_core_cases.FACTOR), relative to the output's max-abs.

The shapes are the smallest at which the kernel can still go wrong.  A chunk is 64 hiddens, so L sits on both sides of 64 / 128 / 192 /
256 and at the cap of 1024.  In the block-per-row form (M <= 2048 and D <= 512) wave w owns the hiddens l = w, w + 4, ...: L % 4 takes
every value, L = 257 gives wave 0 a second chunk (65 hiddens) and the others none, L = 3 leaves wave 3 without any hidden, and at the
cap every wave walks four full chunks.  D covers every ITER (<= 256 / <= 512 / <= 1024) and ragged D / 4; M = 2048 / 2049 at L = 65 is
the switch between the two forms."""
import attn_core_cases as K

E32 = 1.4e-6                    # measured 1.12e-6 (test_deep_pool_host.py prints every case's)
BOUND = K.FACTOR * E32
FORMS = {f'pool_mix_deep_{r}kernel<{it}{b}>' for r in ('', 'rows_') for it in (1, 2, 4) for b in ('', ',bf16') if not (r and it == 4)}


def _dpm(D, L, M, kb, i):
    """attn_core_cases._pm with the forms of the chunked launcher (same rule: by M and D alone); the flags alternate as there"""
    c = K._pm(D, L, M, kb, i)
    c['form'] = c['form'].replace('pool_mix_', 'pool_mix_deep_')
    c['name'] = 'deep-' + c['name'][len('pool-'):]
    return c


def _cases():
    pairs = [(64, 65), (64, 128), (64, 257), (96, 66), (96, 127), (96, 193), (256, 129), (256, 191), (256, 128), (320, 65), (320, 129), (320, 257),
             (512, 66), (512, 127), (512, 191), (768, 65), (768, 128), (768, 193), (1024, 66), (1024, 129), (1024, 257),
             (96, 3)]                                         # (wave 3 of the block-per-row form without a hidden)
    cs = []
    for i, (D, L) in enumerate(pairs):
        for kb in (0, 1):
            cs.append(_dpm(D, L, (1, 5)[(i + kb) % 2], kb, i + kb))
    # the cap, at small D and M only
    for i, (D, L, M) in enumerate([(64, 1023, 1), (64, 1024, 1), (512, 1024, 2), (512, 1023, 2), (1024, 1023, 1), (1024, 1024, 1)]):
        for kb in (0, 1):
            cs.append(_dpm(D, L, M, kb, i + kb))
    # the switch between the forms at M = 2048 / 2049 (D <= 512: the wave-per-row form's ITER 1 and 2 are reached above 2048 rows only)
    for i, (D, M, kb) in enumerate([(64, 2048, 0), (64, 2049, 0), (64, 2049, 1), (260, 2049, 0), (260, 2049, 1)]):
        cs.append(_dpm(D, 65, M, kb, i))
    for k, c in enumerate(cs):
        c['seed'] = 12000 + k
    return cs


DEEP = _cases()


def deep_expect(c, d, **kw):
    """attn_core_cases.pool_expect: the reference on the values the chosen form reads (that function tells the wave-per-row form, which
    reads the hiddens' bf16 image, by the name of d4_pool_mix's kernel)"""
    return K.pool_expect(dict(c, form=c['form'].replace('pool_mix_deep_', 'pool_mix_')), d, **kw)


# the engine configurations of the oracle comparisons (keyword arguments of util.small_model on top of wide_frames=True): 2 depth + 1 pooled
# hiddens at the final pool, 2 p + 3 at the in-loop pool p
ENGINE = dict(
    A=dict(depth=32, time_block_every=4),                                                        # dim 64; L = 65 at the last in-loop pool and the final pool
    B=dict(depth=33, time_block_every=2, dim=32, attn_dim_head=16, attn_heads=3, num_tasks=0),
    C=dict(depth=40, dim=320),                                                                   # ragged ITER = 2
    D=dict(depth=65, time_block_every=8, dim=32, attn_heads=1, attn_dim_head=32),                # L up to 131: three chunks
)
