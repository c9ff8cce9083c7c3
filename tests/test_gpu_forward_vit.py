"""VTAMIQ.forward_vit on the MI355X: the reference's own forward_vit goldens in every precision mode, shapes, bit-identity with the
scoring path's token trace, the attention-probability kernel at full size and at S = 5001, and its masking."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests.gpu_util import stream, to_planes
from tests.test_forward_vit_layout import load_vit_case
from vtamiq_amd import VTAMIQ, _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_MODES = ["fp16x3", "bf16x3", "fp16x2", "fp16", "bf16"]
THREE_TERM_ATTENTION = ("fp16x3", "bf16x3", "fp16x2")       # the attention products of fp16x2 are 3-term
# x and hidden_states: the per-mode bounds of tests/test_gpu_parity.py::test_token_trace_c1 (max abs error / max |ref|)
STATE_TOL = {"fp16x3": 2e-5, "fp16x2": 1e-3, "bf16x3": 2e-4, "fp16": 5e-3, "bf16": 4e-2}
# attn_weights against the reference, absolute: the 3-term bounds as specified, the others about 3 - 4x the observed maxima
# (profiles/r07_vit_probe.txt: fp16x3 3.4e-7, bf16x3 7.1e-7, fp16x2 3.4e-5, fp16 4.7e-5, bf16 4.5e-4)
PROB_TOL = {"fp16x3": 1e-5, "bf16x3": 1e-4, "fp16x2": 1e-4, "fp16": 2e-4, "bf16": 2e-3}
# attn_weights against an fp64 softmax of the engine's own layer input (encoder drift removed), absolute; observed at B = 4, N = 500:
# fp16x3 4.8e-8, bf16x3 1.2e-7, fp16x2 3.8e-6, fp16 6.4e-6, bf16 4.5e-5
PROB_LOCAL_TOL = {"fp16x3": 1e-5, "bf16x3": 1e-5, "fp16x2": 2e-5, "fp16": 5e-5, "bf16": 3e-4}


def build(kw, sd_np, precision, layers=False, attention=False):
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    m = m.to(DEV).eval()
    m.transformer.encoder.return_layers = layers            # set after construction, as a reference user may
    m.transformer.encoder.return_attention = attention
    return m


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("precision", ALL_MODES)
@pytest.mark.parametrize("name", ["vit_b2_n29", "vit_b2_n20"])
def test_against_reference_goldens(name, precision):
    g, kw, spec, sd, (patches, pos, scales) = load_vit_case(name)
    m = build(kw, sd, precision, layers=True, attention="probs" in g)
    T = spec.num_tokens
    with torch.no_grad():
        x, attn, hid = m.forward_vit(cuda(patches), cuda(pos), cuda(scales), tokens_only=False)
        x_t, attn_t, hid_t = m.forward_vit(cuda(patches), cuda(pos), cuda(scales), tokens_only=True)
    torch.cuda.synchronize()
    tol = STATE_TOL[precision]
    ex = rel(x.cpu().numpy(), g["x_all"])
    assert ex < tol, ("x", ex)
    assert torch.equal(x_t, x[:, :T])
    states = g["states_all"][:, :, :T] if "states_all" in g else g["states_tok"]
    errs = [rel(h.cpu().numpy(), states[i]) for i, h in enumerate(hid_t)]
    if "states_all" in g:
        errs += [rel(h.cpu().numpy(), g["states_all"][i]) for i, h in enumerate(hid)]
    print(f"{name} {precision}: x {ex:.2e}, states max {max(errs):.2e}")
    assert max(errs) < tol, errs
    if "probs" in g:
        pe = [float((a.cpu().double() - torch.from_numpy(g["probs"][i]).double()).abs().max()) for i, a in enumerate(attn)]
        print(f"{name} {precision}: attn_weights max abs error {max(pe):.2e}")
        assert max(pe) <= PROB_TOL[precision], pe
        if precision in THREE_TERM_ATTENTION:
            for a in attn:
                assert float((a.double().sum(-1) - 1.0).abs().max()) <= 1e-5
        for a, b in zip(attn, attn_t):
            assert torch.equal(a, b)


@pytest.mark.parametrize("tokens_only", [True, False])
@pytest.mark.parametrize("layers", [False, True])
@pytest.mark.parametrize("attention", [False, True])
def test_shapes_dtypes_and_list_lengths(tokens_only, layers, attention):
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=3, num_extra_tokens=1, pretrained=False))
    m = VTAMIQ(**kw, precision="fp16x3")
    sd = synth.make_state_dict(m.spec, 5)
    m = build(kw, sd, "fp16x3", layers, attention)
    B, N = 3, 40
    patches, pos, _ = synth.make_inputs(m.spec, B, N, 6)
    with torch.no_grad():
        x, attn, hid = m.forward_vit(cuda(patches[:, 0]), cuda(pos[:, 0]), None, tokens_only=tokens_only)
    T, S, H, L = 2, N + 2, 768, 3
    R = T if tokens_only else S
    assert x.shape == (B, R, H) and x.dtype == torch.float32 and x.device.type == "cuda"
    assert len(hid) == (L if layers else 0) and len(attn) == (L if attention else 0)
    for h in hid:
        assert h.shape == (B, R, H) and h.dtype == torch.float32
    for a in attn:
        assert a.shape == (B, 12, S, S) and a.dtype == torch.float32
    assert torch.isfinite(x).all()


@pytest.mark.parametrize("precision", ALL_MODES)
def test_states_equal_the_scoring_paths_token_trace_bitwise(precision):
    """forward_vit(ref images) hidden_states == the ref rows of forward(..., _trace=buf), bit for bit, every layer."""
    g, kw, spec, sd, _ = load_vit_case("vit_b2_n29")
    m = build(kw, sd, precision, layers=True)
    B, N, L, T, H = 2, 29, spec.num_layers, spec.num_tokens, spec.hidden_size
    patches, pos, scales = synth.make_inputs(spec, B, N, 71, aligned=False)
    p, ps = cuda(patches), cuda(pos)
    sc = cuda(scales.astype(np.float32))
    trace = torch.zeros(L + 1, 2 * B, T, H, device=DEV)
    with torch.no_grad():
        m((p[:, 0].contiguous(), p[:, 1].contiguous()), (ps[:, 0].contiguous(), ps[:, 1].contiguous()),
          (sc[:, 0].contiguous(), sc[:, 1].contiguous()), _trace=trace)
        _, _, hid = m.forward_vit(p[:, 0].contiguous(), ps[:, 0].contiguous(), sc[:, 0].contiguous(), tokens_only=True)
    for i in range(L):
        assert torch.equal(hid[i], trace[i + 1, :B]), (precision, i, float((hid[i] - trace[i + 1, :B]).abs().max()))


@pytest.mark.parametrize("precision", ["fp16x3", "bf16"])
def test_requesting_states_and_probs_does_not_change_x(precision):
    g, kw, spec, sd, (patches, pos, scales) = load_vit_case("vit_b2_n29")
    m = build(kw, sd, precision)
    with torch.no_grad():
        x0, a0, h0 = m.forward_vit(cuda(patches), cuda(pos), cuda(scales), tokens_only=False)
        m.transformer.encoder.return_layers = True
        m.transformer.encoder.return_attention = True
        x1, a1, h1 = m.forward_vit(cuda(patches), cuda(pos), cuda(scales), tokens_only=False)
    assert a0 == [] and h0 == [] and len(a1) == spec.num_layers and len(h1) == spec.num_layers
    assert torch.equal(x0, x1)


def _local_probs(sd, spec, x_in, layer, rows=None):
    """fp64 softmax(Q K^T / 8) of layer `layer` on the layer input x_in (B, S, H) (query rows `rows` of each sequence, default all)."""
    p = f"transformer.encoder.layers.{layer}."
    x = x_in.double()
    ln = torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[p + "attention_norm.weight"].double(), sd[p + "attention_norm.bias"].double(), 1e-6)
    B, S, H = ln.shape
    nh = spec.num_heads

    def proj(nm, a):
        y = a @ sd[f"{p}attn.{nm}.weight"].double().t() + sd[f"{p}attn.{nm}.bias"].double()
        return y.view(B, -1, nh, 64).permute(0, 2, 1, 3)
    q = proj("query", ln if rows is None else ln[:, rows])
    k = proj("key", ln)
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)


@pytest.mark.parametrize("precision", ALL_MODES)
def test_probs_at_full_size_against_fp64_on_the_engines_layer_input(precision):
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False))
    m0 = VTAMIQ(**kw)
    sd_np = synth.make_state_dict(m0.spec, 9)
    spec = m0.spec
    m = build(kw, sd_np, precision, layers=True, attention=True)
    B, N = 4, 500
    patches, pos, _ = synth.make_inputs(spec, B, N, 10)
    with torch.no_grad():
        _, attn, hid = m.forward_vit(cuda(patches[:, 0]), cuda(pos[:, 0]), None, tokens_only=False)
    sd = {k: v.to(DEV) for k, v in O.to_torch(sd_np).items()}
    with torch.no_grad():
        x0 = O.embeddings(sd, spec, cuda(patches[:, 0]), cuda(pos[:, 0]), None)
    errs = []
    for layer, x_in in enumerate([x0, hid[0]]):
        ref = _local_probs(sd, spec, x_in, layer)
        errs.append(float((attn[layer].double() - ref).abs().max()))
    print(f"full size {precision}: attn_weights vs fp64 on the engine's layer input, max abs {max(errs):.2e}")
    assert max(errs) <= PROB_LOCAL_TOL[precision], errs
    if precision in THREE_TERM_ATTENTION:
        for a in attn:
            assert float((a.double().sum(-1) - 1.0).abs().max()) <= 1e-5


def test_probs_at_5001_tokens():
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False))
    m0 = VTAMIQ(**kw)
    sd_np = synth.make_state_dict(m0.spec, 11)
    spec = m0.spec
    m = build(kw, sd_np, "fp16x3", attention=True)
    B, N = 1, 5000
    patches, pos, _ = synth.make_inputs(spec, B, N, 12)
    with torch.no_grad():
        _, attn, _ = m.forward_vit(cuda(patches[:, 0]), cuda(pos[:, 0]), None, tokens_only=True)
    a = attn[0]
    assert a.shape == (1, 12, 5001, 5001)
    assert float((a.double().sum(-1) - 1.0).abs().max()) <= 1e-5
    rows = torch.from_numpy(np.random.default_rng(13).choice(5001, size=64, replace=False)).to(DEV)
    sd = {k: v.to(DEV) for k, v in O.to_torch(sd_np).items()}
    with torch.no_grad():
        x0 = O.embeddings(sd, spec, cuda(patches[:, 0]), cuda(pos[:, 0]), None)
        ref = _local_probs(sd, spec, x0, 0, rows=rows)
    err = float((a[:, :, rows].double() - ref).abs().max())
    print(f"S = 5001 fp16x3: 64 sampled rows vs fp64, max abs {err:.2e}")
    assert err <= PROB_LOCAL_TOL["fp16x3"]


# vtq_k_attention_probs against an fp64 softmax of the planes' own Q / K, absolute: {3-term format: bound} (also tests/test_gpu_footprint.py)
PROBS_TOL = {True: 1e-5, False: 2e-3}


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
def test_probs_kernel_masks_and_stays_in_bounds(fmt):
    """Three packed sequences of S = 37 (not a multiple of 32 or 64): NaN rows behind the last sequence are never read, no element past
    the (3, 12, 37, 37) output is written, and the values are an fp64 softmax of the planes' own Q / K.
    The key mask itself is pinned at every seam length, on keys that dominate, in tests/test_gpu_attention_seams.py."""
    lib = _lib.load()
    nseq, S, H = 3, 37, 768
    rows = nseq * S
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(rows + 64, 3 * H, generator=g) * 0.5
    three = fmt.endswith("x3")
    scale = 0.125 * math.log2(math.e) if three else 1.0
    qkv[:, :H] *= scale                                        # 3-term: Q in log2 units, as the engine's query projection makes it
    qkv[rows:] = float("nan")                                  # canary rows: a read past the last sequence poisons its outputs
    planes = to_planes(qkv.to(DEV), fmt)
    n = nseq * 12 * S * S
    out = torch.full((n + 64,), float("nan"), device=DEV)
    _lib.check(lib.vtq_k_attention_probs(planes.data_ptr(), planes[0].numel(), out.data_ptr(), nseq, S, S, H, _lib.NUM[fmt], int(three), stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[n:]).all(), "an element past the output was written"
    got = out[:n].view(nseq, 12, S, S).double()
    assert torch.isfinite(got).all()
    v = planes[0].double() + (planes[1].double() if planes.shape[0] == 2 else 0)
    q = v[:rows, :H].view(nseq, S, 12, 64).permute(0, 2, 1, 3) / scale
    k = v[:rows, H:2 * H].view(nseq, S, 12, 64).permute(0, 2, 1, 3)
    ref = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    assert float((got - ref).abs().max()) <= PROBS_TOL[three]


def test_out_of_range_position_and_missing_scales_raise_as_forward_does():
    g, kw, spec, sd, (patches, pos, scales) = load_vit_case("vit_b2_n29")
    m = VTAMIQ(**json.loads(json.dumps(kw)))                   # precision "auto": the error word is read after every call
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).eval()
    bad = pos.copy()
    bad[0, 3, 1] = 1.0
    with torch.no_grad():
        with pytest.raises(IndexError):
            m.forward_vit(cuda(patches), cuda(bad), cuda(scales))
        with pytest.raises(ValueError, match="Model uses scale embedding but scales is passed as None."):
            m.forward_vit(cuda(patches), cuda(pos), None)
        x, _, _ = m.forward_vit(cuda(patches), cuda(pos), cuda(scales))       # the engine is healthy afterwards
    assert torch.isfinite(x).all()
