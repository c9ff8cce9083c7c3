"""CPU-side checks of VTAMIQ.forward_vit (backbone.py:54-60): the ABI 10 entry points are declared and bound, the test oracle that the GPU
tests (tests/test_gpu_forward_vit.py) compare against reproduces the reference's own forward_vit goldens, and the Python-level refusals
come before any device is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests.helpers import GOLDEN
from vtamiq_amd import VTAMIQ, _lib, synth
from vtamiq_amd.spec import make_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_vit_case(name):
    """(golden dict, ctor kwargs, spec, numpy state dict, (patches, pos, scales) of image 0 of each item)."""
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    kw = json.loads(str(g["kwargs"]))
    spec = make_spec(**json.loads(json.dumps(kw)))
    sd = synth.make_state_dict(spec, int(g["wseed"]))
    patches, pos, scales = synth.make_inputs(spec, int(g["B"]), int(g["N"]), int(g["iseed"]), aligned=bool(int(g["aligned"])))
    assert np.isclose(float(patches.astype(np.float64).sum()), float(g["fp_patches"]), rtol=0, atol=1e-6), "generator drift"
    assert np.isclose(float(pos.astype(np.float64).sum()), float(g["fp_pos"]), rtol=0, atol=1e-6), "generator drift"
    return g, kw, spec, sd, (patches[:, 0], pos[:, 0], None if scales is None else scales[:, 0].astype(np.float32))


def oracle_vit(sd, spec, patches, pos, scales):
    """forward_vit(tokens_only=False) with return_layers / return_attention from oracle/vtamiq_oracle.py pieces:
    (x_all (B, S, H), states [L x (B, S, H)], probs [L x (B, h, S, S)])."""
    x = O.embeddings(sd, spec, patches, pos, scales)
    states, probs = [], []
    for i in range(spec.num_layers):
        p = f"transformer.encoder.layers.{i}."
        ln1 = O._layer_norm(x, sd[p + "attention_norm.weight"], sd[p + "attention_norm.bias"])
        probs.append(O.attention(sd, p, ln1, spec.num_heads, return_probs=True)[1])
        x = O.encoder_layer(sd, spec, i, x)
        states.append(x)
    x = O._layer_norm(x, sd["transformer.encoder.encoder_norm.weight"], sd["transformer.encoder.encoder_norm.bias"])
    return x, states, probs


def test_abi_declares_and_binds_forward_vit():
    header = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    for name in ("vtq_forward_vit", "vtq_k_attention_probs"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.vtq_forward_vit.argtypes is not None and lib.vtq_k_attention_probs.argtypes is not None


def test_forward_vit_refuses_a_null_handle():
    lib = _lib.load()
    out = (ctypes.c_float * 4)()
    rc = lib.vtq_forward_vit(None, ctypes.addressof(out), 0, ctypes.addressof(out), None, 1, 1, 0, ctypes.addressof(out), None, None, None)
    assert rc != 0
    assert b"vtq_forward_vit" in lib.vtq_last_error()


def test_attention_probs_refuses_a_two_term_format():
    lib = _lib.load()
    rc = lib.vtq_k_attention_probs(None, 0, None, 1, 32, 32, 768, _lib.NUM["fp16x2"], 0, None)
    assert rc != 0 and b"vtq_k_attention_probs" in lib.vtq_last_error()


@pytest.mark.parametrize("name", ["vit_b2_n29", "vit_b2_n20"])
def test_oracle_composition_reproduces_the_reference_goldens(name):
    """The oracle the GPU tests use, pinned to the reference's own forward_vit (tests/golden/make_vit_golden.py)."""
    g, kw, spec, sd_np, (patches, pos, scales) = load_vit_case(name)
    sd = O.to_torch(sd_np)
    with torch.no_grad():
        x, states, probs = oracle_vit(sd, spec, torch.from_numpy(patches), torch.from_numpy(pos),
                                      None if scales is None else torch.from_numpy(scales))
    T = spec.num_tokens

    def close(a, b):
        return float(np.abs(a.numpy() - b).max()) <= 1e-5

    assert close(x, g["x_all"])
    if "states_all" in g:
        assert all(close(s, g["states_all"][i]) for i, s in enumerate(states))
    else:
        assert all(close(s[:, :T], g["states_tok"][i]) for i, s in enumerate(states))
    if "probs" in g:
        assert all(close(p, g["probs"][i]) for i, p in enumerate(probs))


def test_vtamiq_has_forward_vit():
    assert hasattr(VTAMIQ, "forward_vit")


def _model(**vit):
    vc = dict(variant="ViT-B16", num_keep_layers=1, pretrained=False)
    vc.update(vit)
    return VTAMIQ(vit_config=vc).eval()


def test_forward_vit_flags_live_on_the_encoder_and_can_be_set_later():
    with pytest.warns(UserWarning, match="forward_vit"):
        m = _model(return_layers=True)
    enc = m.transformer.encoder
    assert enc.return_layers is True and enc.return_attention is False
    enc.return_attention = True
    assert m.transformer.encoder.return_attention is True


def test_forward_vit_refusals_come_before_the_device_check():
    p = torch.zeros(1, 4, 3, 16, 16)
    pos = torch.zeros(1, 4, 2)
    m = _model()
    m.train()
    with pytest.raises(NotImplementedError, match="eval"):
        m.forward_vit(p, pos, None)
    m.eval()
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor past the refusals: no CPU fallback
        m.forward_vit(p, pos, None)
    ma = _model(num_adapters=2)
    with pytest.raises(NotImplementedError, match="adapter pair 0"):
        ma.forward_vit(p, pos, None, adapter_num=1)
    for ok in (None, -1, 0):                                  # the default selections pass the refusal and reach the device check
        with pytest.raises(RuntimeError, match="MI355X"):
            ma.forward_vit(p, pos, None, adapter_num=ok)


def test_forward_vit_refuses_the_fp8_experiment():
    if not _lib.fp8_available():
        pytest.fail("the fp8 experiment's library is not built (the session fixture builds it)")
    from vtamiq_amd.experimental_fp8 import VTAMIQFp8
    m = VTAMIQFp8(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False)).eval()
    with pytest.raises(NotImplementedError, match="fp8"):
        m.forward_vit(torch.zeros(1, 4, 3, 16, 16), torch.zeros(1, 4, 2), None)
