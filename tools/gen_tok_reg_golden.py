"""Generate the fixtures of the tokenizer's latent regularisers from the REFERENCE itself (build container only, like tools/gen_tok_train_golden.py,
whose helpers this tool imports):

    python tools/gen_tok_reg_golden.py            # needs the reference checkout (oracle/ref_import.py); writes tests/golden/tok_reg.npz (+ parts)

The narrow tokenizer of tools/gen_tok_train_golden.py (CFG_NARROW, the same seed: the weights are asserted equal to weights_tok_train.npz, which the
tests therefore reuse) with latent_sigreg_loss_weight = latent_ortho_loss_weight = latent_consistency_loss_weight = 0.1 and
latent_sigreg_loss_kwargs = dict(num_slices=256); video (2, 3, 3, 16, 24), 6 latents x 8 per frame.

The draws are recorded as tools/gen_tok_train_golden.py records them (same shaping of the patch mask, same choice of seed), plus `sigreg_projs`: the
FIRST (num_slices, dim_latent) randn of a call, the raw draw of the outer forward's SIGReg term (the consistency term's nested forward draws a second
one and discards the loss it feeds).  oracle/shim/einx.py has no `dot`; the one pattern sigreg uses ('k ... d, m d -> k (...) m') is supplied here as
torch.einsum, the way the other tool supplies `where`.  The other tool's `run_case` asserts that every term but `recon` is zero, so the cases here
run through `run_reg_case`, the same procedure with the four terms and their normalisers recorded.

Cases (train() mode): `reg` (loss normalisation on), `reg2` (the next call: the four normaliser states carry over), `reg_nonorm`
(use_loss_normalization False).  Per case: video, the four draws, the four loss terms and the total, latents, recon_video, each normaliser's state
before and after, and the gradient of the total with respect to every parameter tests/tok_train_cases.py::has_gradient admits (asserted non-zero)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gen_tok_train_golden import CFG_NARROW, OUT, recorded_draws, save_parts, unread   # noqa: E402
from oracle.gen_golden import META, _reference_tokenizer, npy                            # noqa: E402
from oracle.ref_import import load_reference                                             # noqa: E402

WEIGHT, NUM_SLICES = 0.1, 256
REG_KW = dict(latent_sigreg_loss_weight=WEIGHT, latent_ortho_loss_weight=WEIGHT, latent_consistency_loss_weight=WEIGHT,
              latent_sigreg_loss_kwargs=dict(num_slices=NUM_SLICES))
TERMS = ('recon', 'latent_ortho', 'latent_consistency', 'latent_sigreg')
NORMALIZERS = {f: f'{f}_loss_normalizer' for f in TERMS}


class recorded_reg_draws:
    """recorded_draws plus the SIGReg projections and the einx.dot pattern of sigreg"""
    def __init__(self, D4, rec):
        self.D4, self.rec, self.inner = D4, rec, recorded_draws(D4, rec)

    def __enter__(self):
        import einx
        self.inner.__enter__()
        D4, rec = self.D4, self.rec
        self.saved = (D4.randn, getattr(einx, 'dot', None))

        def randn(*a, **k):
            r = self.saved[0](*a, **k)
            if 'sigreg_projs' not in rec and tuple(r.shape) == (NUM_SLICES, CFG_NARROW['dim_latent']):
                rec['sigreg_projs'] = r.clone()
            return r

        def dot(pattern, x, y):
            assert pattern == 'k ... d, m d -> k (...) m', pattern
            return torch.einsum('knd,md->knm', x.reshape(x.shape[0], -1, x.shape[-1]), y)

        D4.randn, einx.dot = randn, dot

    def __exit__(self, *exc):
        import einx
        self.D4.randn, einx.dot = self.saved
        return self.inner.__exit__(*exc)


def norm_states(tok):
    return {f: (getattr(tok, m).exp_avg_sq.detach().clone() if getattr(tok, m, None) is not None else torch.ones(1)) for f, m in NORMALIZERS.items()}


def run_reg_case(D4, tok, out, name, x, seed0):
    """One training forward + backward with the three terms on, under recorded draws; the seed is the first from seed0 on whose time_indices are not all 0."""
    lat = {}
    def keep_first(m, a, o):                                           # the outer forward's latents; the consistency term's nested forward calls it again
        if 'latents' not in lat:
            lat['latents'] = o.detach().tanh()

    hook = tok.encoded_to_latents.register_forward_hook(keep_first)
    before = norm_states(tok)
    try:
        for seed in range(seed0, seed0 + 64):
            rec = {}
            lat.clear()
            with torch.no_grad():
                for f, m in NORMALIZERS.items():
                    if getattr(tok, m, None) is not None and tok.use_loss_normalization:
                        getattr(tok, m).exp_avg_sq.copy_(before[f])
            tok.zero_grad()
            torch.manual_seed(seed)
            with recorded_reg_draws(D4, rec):
                total, (losses, recon_video) = tok(x, return_intermediates=True)
            if bool(rec['time_indices'].any()):
                break
        else:
            raise AssertionError('no seed with a non-zero time index')
    finally:
        hook.remove()
    total.backward()
    for k in ('patch_mask', 'time_indices', 'noise', 'sigreg_projs'):
        out[f'{name}_{k}'] = npy(rec[k])
    out[f'{name}_video'], out[f'{name}_seed'] = npy(x), np.array(seed)
    out[f'{name}_total'], out[f'{name}_latents'], out[f'{name}_recon_video'] = npy(total.reshape(())), npy(lat['latents']), npy(recon_video)
    for f in losses._fields:
        v = float(getattr(losses, f))
        if f in TERMS:
            assert v > 0., (name, f, v)
            out[f'{name}_{f}'] = npy(getattr(losses, f).reshape(()))
        else:
            assert v == 0., (name, f, v)
    after = norm_states(tok)
    for f in TERMS:
        out[f'{name}_norm_before/{f}'], out[f'{name}_norm_after/{f}'] = npy(before[f]), npy(after[f])
    ng = 0
    for k, p in tok.named_parameters():
        if unread(k):
            assert p.grad is None or float(p.grad.abs().max()) == 0., k
            continue
        assert p.grad is not None and float(p.grad.abs().max()) > 0., f'{name}: no gradient on {k}'
        out[f'{name}_grad/{k}'] = npy(p.grad); ng += 1
    print(name, 'seed', seed, {f: float(getattr(losses, f)) for f in TERMS}, 'total', float(total), 'time_indices', rec['time_indices'].tolist(), 'grads', ng,
          'norm', {f: v.tolist() for f, v in after.items()})


def main():
    D4 = load_reference()
    tok, g = _reference_tokenizer(D4, dict(CFG_NARROW, **REG_KW), 81)
    tok.train()
    with torch.no_grad():
        tok.mask_token.mul_(30.)                                       # as tools/gen_tok_train_golden.py::gen_narrow
    have = {}
    for f in sorted(os.listdir(OUT)):
        if f == 'weights_tok_train.npz' or (f.startswith('weights_tok_train.p') and f.endswith('.npz')):
            z = np.load(os.path.join(OUT, f))
            have.update({k: z[k] for k in z.files})
    for k, v in tok.state_dict().items():
        if 'loss_normalizer' not in k and v.numel() > 0:
            assert np.array_equal(have[k], npy(v.detach().float())), f'{k}: not the weights of weights_tok_train.npz'
    video = torch.rand(2, 3, 3, 16, 24, generator=g)
    out = {}
    run_reg_case(D4, tok, out, 'reg', video, 700)
    run_reg_case(D4, tok, out, 'reg2', video, 800)
    tok.use_loss_normalization = False
    run_reg_case(D4, tok, out, 'reg_nonorm', video, 900)
    out['cfg_weight'], out['cfg_num_slices'] = np.array(WEIGHT), np.array(NUM_SLICES)
    n = save_parts('tok_reg.npz', {**out, **{'meta_' + k: np.array(v) for k, v in META.items()}})
    print('tok_reg: fixture in', n, 'file(s)')


if __name__ == '__main__':
    main()
