"""CPU: the noise envelope that bounds the bf16 training arithmetic (tests/bf16_emulation.py) is honest — the oracle's own four bf16
variants stay inside it.  Leave-one-out on train.npz: every variant's distance from the fixture, per gradient tensor, is at most 3 x the
largest distance of the other three (measured: 2.45 x at worst, a 2-element bias), all gradients concatenated at most 1.25 x (measured
1.01 x), every loss term at most 3 x + the fp32 loss tolerance.  These are the margins the GPU run (a fifth draw) is held to."""
import torch

import bf16_emulation as emu


def test_emulation_rounds_operands_and_output_gradient_only():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 7, 24, generator=g, requires_grad=True)
    w = torch.randn(32, 24, generator=g, requires_grad=True)
    dy = torch.randn(5, 7, 32, generator=g)
    r = lambda t: t.to(torch.bfloat16).float()
    with emu.bf16_linears():
        y = x @ w.t()
        attn = torch.einsum('bid,bjd->bij', x, x)               # not a Linear: untouched
    y.backward(dy)
    assert torch.equal(y, r(x) @ r(w).t())
    assert torch.equal(attn, torch.einsum('bid,bjd->bij', x, x))
    assert torch.allclose(x.grad, r(dy) @ r(w), atol=1e-5)
    assert torch.allclose(w.grad, (r(dy).reshape(-1, 32).t() @ r(x).reshape(-1, 24)), atol=1e-4)
    with emu.bf16_linears(min_out=64):                          # below the width rule: plain fp32
        assert torch.equal(x @ w.t(), torch.matmul(x, w.t()))
    assert torch.equal(x @ w.t(), torch.matmul(x, w.t()))       # and the operator is restored


def test_the_oracle_stays_inside_its_own_envelope_on_train_npz():
    run, ref = emu.train_fixture('shortcut')
    outs = emu.run_variants(run)
    gkeys = [k for k in ref if k.startswith('grad/')]
    assert len(gkeys) >= 90
    worst_t, worst_g = 0., 0.
    for i, o in enumerate(outs):
        others = [x for j, x in enumerate(outs) if j != i]
        for k in gkeys:
            d, e = emu.rel_l2(o[k], ref[k]), max(emu.rel_l2(x[k], ref[k]) for x in others)
            worst_t = max(worst_t, d / e)
            assert d <= 3. * e + 1e-3, (i, k, d, e)
        d, e = emu.global_rel_l2(o, ref, gkeys), max(emu.global_rel_l2(x, ref, gkeys) for x in others)
        worst_g = max(worst_g, d / e)
        assert d <= 1.25 * e, (i, d, e)
        for k in ('loss/flow', 'loss/shortcut'):
            d = abs(float(o[k]) - float(ref[k]))
            e = max(abs(float(x[k]) - float(ref[k])) for x in others)
            assert d <= 3. * e + 1e-5 * abs(float(ref[k])), (i, k, d, e)
    print(f'leave-one-out: worst per-tensor ratio {worst_t:.2f}, worst global ratio {worst_g:.3f}')
    # the bf16 variants really differ from fp32 (the envelope is not vacuous) and from each other
    E, G, L, _ = emu.model_envelope(run, ref)
    assert 1e-3 < G < 5e-2 and min(E.values()) > 1e-4
