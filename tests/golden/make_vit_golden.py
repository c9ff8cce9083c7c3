#!/usr/bin/env python3
"""Capture the forward_vit golden vectors from the REFERENCE ITSELF (backbone.py:54-60, transformer.py:628-641, 363-378).

Same recipe as make_golden.py (whose helpers this imports, unchanged): weights and inputs regenerated from seeds by vtamiq_amd.synth,
loaded into the reference's VTAMIQ (a VisionTransformerBackbone) with return_layers=True and return_attention=True, and the outputs of
its own forward_vit stored.  The all-token outputs are stored once; the generator checks that the reference's tokens_only=True call
returns exactly their [:, :T] slices.

Run:  python tests/golden/make_vit_golden.py        (writes tests/golden/vit_*.npz)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                          # noqa: E402  (also puts the repository root on sys.path)

from vtamiq_amd import synth                      # noqa: E402
from vtamiq_amd.spec import make_spec             # noqa: E402


def run_vit_case(name, vtamiq_kwargs, B, N, wseed, iseed, aligned=True, keep_probs=True, keep_states_all=True):
    """One image per item: image 0 of synth.make_inputs' pairs.  Stores x_all (B, S, H); states_all (L, B, S, H) or states_tok
    (L, B, T, H); probs (L, B, h, S, S) when keep_probs."""
    kw = json.loads(json.dumps(vtamiq_kwargs))
    spec = make_spec(**json.loads(json.dumps(kw)))
    kw.setdefault("vit_config", {}).update(return_layers=True, return_attention=True)
    model = mg.build_reference(kw)
    mg.load_seeded(model, spec, wseed)
    patches, pos, scales = synth.make_inputs(spec, B, N, iseed, aligned=aligned)
    p = torch.from_numpy(patches)[:, 0].clone()
    ps = torch.from_numpy(pos)[:, 0].clone()
    sc = torch.from_numpy(scales)[:, 0].to(torch.float32).clone() if scales is not None else None
    T = spec.num_tokens
    with torch.no_grad():
        x_all, attn_all, hid_all = model.forward_vit(p, ps, sc, tokens_only=False)
        x_tok, attn_tok, hid_tok = model.forward_vit(p, ps, sc, tokens_only=True)
    L = spec.num_layers
    assert len(attn_all) == L and len(hid_all) == L and len(attn_tok) == L and len(hid_tok) == L
    # tokens_only=True is the [:, :T] slice of the all-token call, bit for bit (transformer.py:632-636)
    assert torch.equal(x_tok, x_all[:, :T])
    for a, b in zip(hid_tok, hid_all):
        assert torch.equal(a, b[:, :T])
    for a, b in zip(attn_tok, attn_all):
        assert torch.equal(a, b)
    out = dict(kwargs=json.dumps(vtamiq_kwargs), B=B, N=N, wseed=wseed, iseed=iseed, aligned=int(aligned))
    out["x_all"] = x_all.numpy().astype(np.float32)
    if keep_states_all:
        out["states_all"] = torch.stack(hid_all).numpy().astype(np.float32)
    else:
        out["states_tok"] = torch.stack(hid_tok).numpy().astype(np.float32)
    if keep_probs:
        out["probs"] = torch.stack(attn_all).numpy().astype(np.float32)
    out["fp_patches"] = np.float64(patches.astype(np.float64).sum())
    out["fp_pos"] = np.float64(pos.astype(np.float64).sum())
    np.savez(os.path.join(HERE, f"{name}.npz"), **out)
    print(f"{name}: " + ", ".join(f"{k} {v.shape}" for k, v in out.items() if isinstance(v, np.ndarray) and v.ndim > 0))


def main():
    sys.path.insert(0, mg.REF)
    mg._install_stubs()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    B16 = "ViT-B16"
    run_vit_case("vit_b2_n29", dict(vit_config=dict(variant=B16, num_keep_layers=2, num_extra_tokens=2, num_scales=2, use_layer_scale=True)),
                 B=2, N=29, wseed=61, iseed=62, aligned=False)
    run_vit_case("vit_b2_n20", dict(vit_config=dict(variant=B16)), B=2, N=20, wseed=63, iseed=64, keep_probs=False, keep_states_all=False)


if __name__ == "__main__":
    main()
