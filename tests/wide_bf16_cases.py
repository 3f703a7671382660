"""Operator cases of the bf16-product wide attention core (csrc/attn_wide_bf16.hip: wide_attn_bf16_kernel<DH>, reached through
d4_small_attn_wide_bf16), shared by tests/test_gpu_wide_bf16.py (the kernel against float64) and tests/test_wide_bf16_host.py (the
same inputs on the CPU).  The table is wide_infer_cases.WIDE with the forms renamed and seeds of its own, plus the cases the host
test's mutation rule needs (a second case with ten or more special items, where one wrongly visible key or one wrongly masked row
is large against bf16 rounding).

The tolerance.  The reference is the EXACT float64 attn_core_ref.small_attn_ref.  E16 is the largest rel_err against it of the
contract's emulation (wide_bf16_ref.py) over these cases and four variants — key tile 64 and 16, float64 and float32 arithmetic —
measured on the CPU and recorded here with a quarter of headroom (test_wide_bf16_host.py asserts it still holds).  The kernel differs
from the float32 tile-64 emulation in summation order and the device's tanhf / expf only, but either can flip a bf16 rounding of q,
k', v' or p: BOUND16 = 2 x E16 pays for that (the variants differ from one another by about 0.3 x E16)."""
import wide_infer_cases as W

E16 = 7.3e-3                     # measured 5.8e-3 (cross-65x64), x 1.25
BOUND16 = 2 * E16


def _form(dh):
    return f'wide_attn_bf16_kernel<{dh}>'


def _cases():
    import attn_core_cases as K
    cs = [dict(c, form=_form(c['dh'])) for c in W.WIDE]
    cs.append(K._sa('special-90-ms12', _form(64), 90, 90, 64, G=2, H=2, vres=1, ms=12, belief=1, clamp=3.))
    cs.append(K._sa('special-75-ms11-dh16', _form(16), 75, 75, 16, G=2, H=2, vres=0, ms=11, belief=1))
    for k, c in enumerate(cs):
        c['seed'] = 7000 + k
    return cs


WIDE16 = _cases()

ENGINE = W.ENGINE
