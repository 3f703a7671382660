"""Write tests/golden/muon_names.json from the REFERENCE itself (build container only, like oracle/gen_golden.py):

    python tools/gen_muon_names.py          # needs the reference checkout (oracle/ref_import.py)

For one small DynamicsWorldModel (with actions, depth 4 and a time block every 2 layers, so time layers are in) and one small VideoTokenizer the
file holds the constructor kwargs and the sorted `named_parameters()` keys of the tensors `muon_parameters()` returns.  Names only: no weights,
no code.  tests/test_muon_host.py compares `muon_parameters()` of the mirrors built from the same kwargs against it."""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness                                     # noqa: E402,F401  (the reference harness: import path set-up)
from oracle.ref_import import load_reference                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'muon_names.json')

DYNAMICS = dict(dim=64, dim_latent=8, num_latent_tokens=6, depth=4, time_block_every=2, attn_heads=2, num_discrete_actions=4, num_tasks=3)
TOKENIZER = dict(dim=32, dim_latent=8, patch_size=4, image_height=16, image_width=24, num_latent_tokens=6, encoder_depth=2, decoder_depth=2,
                 time_block_every=2, attn_heads=2, attn_dim_head=64, channels=3, decoder_flow_steps=2, lpips_loss_weight=0.)


def names_of(model):
    by_id = {id(p): k for k, p in model.named_parameters()}
    muon = model.muon_parameters()
    assert len({id(p) for p in muon}) == len(muon), 'muon_parameters() names a tensor twice'
    assert all(p.ndim == 2 for p in muon)
    return sorted(by_id[id(p)] for p in muon)


def main():
    D4 = load_reference()
    torch.manual_seed(0)
    out = {
        'dynamics': dict(kwargs=DYNAMICS, names=names_of(D4.DynamicsWorldModel(**DYNAMICS))),
        'tokenizer': dict(kwargs=TOKENIZER, names=names_of(D4.VideoTokenizer(**TOKENIZER))),
    }
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    for k, v in out.items():
        print(k, len(v['names']), 'muon parameters')


if __name__ == '__main__':
    main()
