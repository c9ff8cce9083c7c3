"""VTAMIQ.forward_rollout on the MI355X: scores plus the attention rollout of the consumed token, against an fp64 evaluation of the
definition on the attention maps forward_vit(return_attention=True) returns for the same model and the same images (each side on its own).
Those maps are pinned against reference-captured goldens in tests/test_gpu_forward_vit.py; the code under test is never its own reference.

Gates: absolute, per numerics mode, 4 x the maximum error observed on the MI355X over every test of this file that uses them (the margin
PROB_TOL of tests/test_gpu_forward_vit.py keeps over its observed maxima), never above that file's PROB_LOCAL_TOL[mode] (PROB_TOL[mode] for
the reference goldens).  Observed maxima (the `measured` lines every test prints):
    rollout against the model's own maps   fp16x3 2.77e-8   bf16x3 1.05e-8   fp16x2 1.38e-8   fp16 1.40e-8   bf16 2.35e-8
        (fp32 rounding of the walk itself: the maps are the same in the code under test and in the reference)
    last_attention against the same maps   0 in every mode and case: with r = e_t the step kernel forms the token's row with the
        arithmetic of attention_probs.hip, so the gate is equality
    against the reference's maps (vit_b2_n29), rollout / last_attention
        fp16x3 1.31e-8 / 1.97e-7   bf16x3 3.14e-8 / 6.63e-7   fp16x2 9.72e-7 / 2.62e-5   fp16 2.02e-6 / 3.74e-5   bf16 1.47e-5 / 2.64e-4
        (fp16x2 last_attention: 4 x 2.62e-5 is above PROB_TOL's 1e-4, so the gate is that cap; these values have the bits of forward_vit's
        maps, whose own test observes 3.4e-5 in this mode under the same cap)
    vtq_k_rollout_step against fp64       fp16x3 3.2e-9   bf16x3 4.4e-9   fp16 3.2e-9   bf16 4.0e-9 (bound: PROBS_TOL, as the issue sets it)
A first version took the last layer's row from the folded CLS tail (fp32 rows against W_k^T q).  Against the maps of the stress case it was
off by 7.4e-6 (fp16x3), 4.0e-5 (bf16x3), 1.9e-3 (fp16), 2.2e-2 (bf16) in last_attention: the fold does not round Q and K to the mode's
operand planes, the maps do.  The engine therefore projects the last layer's Q / K rows in a rollout call and uses the step kernel there too.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests.footprint import Arena
from tests.gpu_util import stream, to_planes
from tests.helpers import GOLDEN, stress_state
from tests.test_forward_vit_layout import load_vit_case
from tests.test_gpu_forward_vit import ALL_MODES, PROB_LOCAL_TOL, PROB_TOL, PROBS_TOL, THREE_TERM_ATTENTION
from vtamiq_amd import VTAMIQ, Rollout, _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 4 x the observed maxima above, capped by PROB_LOCAL_TOL
ROLLOUT_TOL = {"fp16x3": 1.1e-7, "bf16x3": 4.2e-8, "fp16x2": 5.5e-8, "fp16": 5.6e-8, "bf16": 9.4e-8}
LAST_TOL = {"fp16x3": 0.0, "bf16x3": 0.0, "fp16x2": 0.0, "fp16": 0.0, "bf16": 0.0}
# against the rollout of the REFERENCE's own maps (golden vit_b2_n29), capped by PROB_TOL
GOLDEN_ROLLOUT_TOL = {"fp16x3": 5.3e-8, "bf16x3": 1.3e-7, "fp16x2": 3.9e-6, "fp16": 8.1e-6, "bf16": 5.9e-5}
GOLDEN_LAST_TOL = {"fp16x3": 7.9e-7, "bf16x3": 2.7e-6, "fp16x2": 1e-4, "fp16": 1.5e-4, "bf16": 1.06e-3}
for _m in ALL_MODES:
    assert ROLLOUT_TOL[_m] <= PROB_LOCAL_TOL[_m] and LAST_TOL[_m] <= PROB_LOCAL_TOL[_m]
    assert GOLDEN_ROLLOUT_TOL[_m] <= PROB_TOL[_m] and GOLDEN_LAST_TOL[_m] <= PROB_TOL[_m]

STRESS_KW = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=3, num_extra_tokens=1, pretrained=False))


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(kw, sd_np, precision, **extra):
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision=precision, **extra)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return m.to(DEV).eval()


def sides(patches, pos, scales):
    """The collated (B, 2, ...) arrays of synth.make_inputs as forward()'s ((ref, dist), (ref, dist), (ref, dist) | None) on the device."""
    p, ps = cuda(patches), cuda(pos)
    sc = None if scales is None else cuda(scales.astype(np.float32))
    pair = lambda t: (t[:, 0].contiguous(), t[:, 1].contiguous())
    return pair(p), pair(ps), (pair(sc) if sc is not None else None)


def rollout_fp64(maps, t, order=None, head=None):
    """e_t^T A_L ... A_1 with A_l = (I + mean over heads of P_l) / 2, as a row vector in fp64.  maps: L tensors (B, h, S, S).
    order: the layer walk (default last to first); head: one head instead of the mean -- the wrong variants the stress case must see."""
    L = len(maps)
    B, h, S, _ = maps[0].shape
    r = torch.zeros(B, S, dtype=torch.float64, device=maps[0].device)
    r[:, t] = 1.0
    for l in (order if order is not None else range(L - 1, -1, -1)):
        a = torch.zeros(B, S, dtype=torch.float64, device=r.device)
        for hd in (range(h) if head is None else [head]):                     # head by head: no (B, h, S, S) fp64 copy at S = 5001
            a += torch.einsum("bi,bij->bj", r, maps[l][:, hd].double())
        r = 0.5 * r + 0.5 * a / (h if head is None else 1)
    return r


def reference(m, inp, t=0):
    """(rollout (2, B, S), last_attention (2, B, h, S)) in fp64 from the model's own forward_vit maps, each side separately."""
    (pr, pd), (qr, qd), sc = inp
    enc = m.transformer.encoder
    enc.return_attention = True
    roll, last = [], []
    with torch.no_grad():
        for k, (p, q) in enumerate(((pr, qr), (pd, qd))):
            _, maps, _ = m.forward_vit(p, q, None if sc is None else sc[k], tokens_only=True)
            roll.append(rollout_fp64(maps, t))
            last.append(maps[-1][:, :, t, :].double())
            del maps
    enc.return_attention = False
    return torch.stack(roll), torch.stack(last)


def errors(got, ref):
    return float((got.rollout.double() - ref[0]).abs().max()), float((got.last_attention.double() - ref[1]).abs().max())


def check(what, precision, got, ref):
    er, el = errors(got, ref)
    print(f"measured {what} {precision}: rollout {er:.2e} last_attention {el:.2e}")
    assert torch.isfinite(got.rollout).all() and torch.isfinite(got.last_attention).all()
    assert float(got.rollout.min()) > 0 and float(got.last_attention.min()) > 0
    assert er <= ROLLOUT_TOL[precision], (what, precision, er)
    assert el <= LAST_TOL[precision], (what, precision, el)
    if precision in THREE_TERM_ATTENTION:
        assert float((got.rollout.double().sum(-1) - 1.0).abs().max()) <= 1e-5


# ---- the case that can see a bug -------------------------------------------------------------------------------------------
_stress = {}


def stress_case(precision, **extra):
    """Model, inputs and (once per precision, never modified) the fp64 reference of the peaked-attention case: S = 132."""
    spec = VTAMIQ(**STRESS_KW, precision="fp16x3").spec
    if "sd" not in _stress:
        _stress["sd"] = stress_state(spec, 21, qk=5.0)
        _stress["inp"] = sides(*synth.make_inputs(spec, 2, 130, 22))
    m = build(STRESS_KW, _stress["sd"], precision, **extra)
    return m, _stress["inp"]


def stress_reference(precision, t=0):
    key = (precision, t)
    if key not in _stress:
        m, inp = stress_case(precision)
        _stress[key] = reference(m, inp, t)
    return _stress[key]


def test_the_stress_reference_is_far_from_uniform_and_sees_the_layer_order():
    m, inp = stress_case("fp16x3")
    (pr, _), (qr, _), _ = inp
    m.transformer.encoder.return_attention = True
    with torch.no_grad():
        _, maps, _ = m.forward_vit(pr, qr, None, tokens_only=True)
    T = m.spec.num_tokens
    ref = rollout_fp64(maps, 0)
    patch = ref[:, T:]
    ratio = float((patch.max(-1).values / patch.min(-1).values).min())
    wrong = {"reversed": rollout_fp64(maps, 0, order=range(len(maps))), "head 0": rollout_fp64(maps, 0, head=0), "token 1": rollout_fp64(maps, 1),
             "layer skipped": rollout_fp64(maps, 0, order=[2, 0])}
    diffs = {k: float((v - ref).abs().max()) for k, v in wrong.items()}
    print(f"stress reference: patch max/min {ratio:.1f}; wrong variants differ by {diffs}")
    assert ratio >= 10
    assert diffs["reversed"] >= 1e-3


@pytest.mark.parametrize("precision", ALL_MODES)
def test_stress_case(precision):
    m, inp = stress_case(precision)
    with torch.no_grad():
        q, got = m.forward_rollout(*inp)
        q0, _ = m(*inp)
        q2, again = m.forward_rollout(*inp)
    B, S, h = 2, 132, 12
    assert isinstance(got, Rollout) and got.rollout.shape == (2, B, S) and got.last_attention.shape == (2, B, h, S)
    assert got.rollout.dtype == torch.float32 and got.last_attention.dtype == torch.float32 and got.rollout.device.type == "cuda"
    check("stress", precision, got, stress_reference(precision))
    bits = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(bits(q), bits(q0)), "q differs from forward()"
    assert torch.equal(bits(q), bits(q2)) and torch.equal(bits(got.rollout), bits(again.rollout))
    assert torch.equal(bits(got.last_attention), bits(again.last_attention))


@pytest.mark.parametrize("precision", ALL_MODES)
def test_register_token(precision):
    m, inp = stress_case(precision)
    m.token_num = 1
    with torch.no_grad():
        _, got = m.forward_rollout(*inp)
    check("register token", precision, got, stress_reference(precision, 1))
    other = stress_reference(precision, 0)
    assert float((got.rollout.double() - other[0]).abs().max()) > 1e-2         # the token matters in this case


@pytest.mark.parametrize("precision", ["fp16x3", "bf16"])
def test_full_last_layer_option(precision):
    m, inp = stress_case(precision, engine_options=_lib.OPT_FULL_LAST_LAYER)
    with torch.no_grad():
        q, got = m.forward_rollout(*inp)
        q0, _ = m(*inp)
    check("full last layer", precision, got, stress_reference(precision))
    assert torch.equal(q, q0)


def test_a_pairs_values_do_not_depend_on_its_batch():
    spec = VTAMIQ(**STRESS_KW, precision="fp16x3").spec
    m = build(STRESS_KW, stress_state(spec, 21, qk=5.0), "fp16x3")
    (pr, pd), (qr, qd), _ = sides(*synth.make_inputs(spec, 3, 130, 23))
    with torch.no_grad():
        _, full = m.forward_rollout((pr, pd), (qr, qd), None)
        for b in range(3):
            one = slice(b, b + 1)
            _, alone = m.forward_rollout((pr[one], pd[one]), (qr[one], qd[one]), None)
            assert torch.equal(full.rollout[:, one], alone.rollout), b
            assert torch.equal(full.last_attention[:, one], alone.last_attention), b
    assert not torch.equal(full.rollout[:, 0], full.rollout[:, 1])


# ---- more shapes, each against the model's own maps ------------------------------------------------------------------------
SHAPES = {
    "L2 N300": (dict(variant="ViT-B16", num_keep_layers=2), 2, 300, False),                 # S = 301: several query blocks
    "ViT-L N40": (dict(variant="ViT-L16", num_keep_layers=2), 2, 40, False),                # h = 16, H = 1024
    "3 scales N40": (dict(variant="ViT-B16", num_keep_layers=2, num_scales=3), 2, 40, False),
    "pre-embedded N40": (dict(variant="ViT-B16", num_keep_layers=2), 2, 40, True),
    "B4 N500": (dict(variant="ViT-B16", num_keep_layers=2), 4, 500, False),
}


@pytest.mark.parametrize("precision", ["fp16x3", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_more_shapes(shape, precision):
    vit, B, N, tokens = SHAPES[shape]
    kw = dict(vit_config=dict(pretrained=False, **vit))
    spec = VTAMIQ(**kw, precision="fp16x3").spec
    m = build(kw, stress_state(spec, 31, qk=4.0), precision)
    patches, pos, scales = synth.make_inputs(spec, B, N, 32)
    inp = sides(patches, pos, scales)
    if tokens:
        g = torch.Generator(device="cpu").manual_seed(33)
        feats = (torch.randn(B, N, spec.hidden_size, generator=g) * 0.5).to(DEV), (torch.randn(B, N, spec.hidden_size, generator=g) * 0.5).to(DEV)
        inp = (feats, inp[1], inp[2])
    with torch.no_grad():
        q, got = m.forward_rollout(*inp)
        q0, _ = m(*inp)
    assert got.rollout.shape == (2, B, N + spec.num_tokens) and got.last_attention.shape == (2, B, spec.num_heads, N + spec.num_tokens)
    check(shape, precision, got, reference(m, inp))
    assert torch.equal(q, q0)


def test_5001_tokens():
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False))
    spec = VTAMIQ(**kw, precision="fp16x3").spec
    m = build(kw, stress_state(spec, 41, qk=4.0), "fp16x3")
    inp = sides(*synth.make_inputs(spec, 1, 5000, 42))
    with torch.no_grad():
        _, got = m.forward_rollout(*inp)
    assert got.rollout.shape == (2, 1, 5001)
    check("S = 5001", "fp16x3", got, reference(m, inp))          # the reference: fp64 on the GPU, one side and one head at a time


# ---- the reference's own maps ----------------------------------------------------------------------------------------------
# of the two forward_vit goldens, those that hold the reference's attention maps (vit_b2_n20 was captured without them)
GOLDENS_WITH_MAPS = [n for n in ("vit_b2_n29", "vit_b2_n20") if "probs" in np.load(os.path.join(GOLDEN, f"{n}.npz")).files]


@pytest.mark.parametrize("precision", ALL_MODES)
@pytest.mark.parametrize("name", GOLDENS_WITH_MAPS)
def test_against_the_rollout_of_the_reference_goldens_maps(name, precision):
    g, kw, spec, sd, (patches, pos, scales) = load_vit_case(name)
    m = build(kw, sd, precision)
    p, ps, sc = cuda(patches), cuda(pos), cuda(scales)
    with torch.no_grad():
        _, got = m.forward_rollout((p, p), (ps, ps), None if sc is None else (sc, sc))        # the golden's image on both sides
    maps = [torch.from_numpy(a).to(DEV) for a in g["probs"]]
    ref = rollout_fp64(maps, 0)
    last = maps[-1][:, :, 0, :].double()
    er = max(float((got.rollout[k].double() - ref).abs().max()) for k in (0, 1))
    el = max(float((got.last_attention[k].double() - last).abs().max()) for k in (0, 1))
    print(f"measured golden {name} {precision}: rollout {er:.2e} last_attention {el:.2e}")
    assert er <= GOLDEN_ROLLOUT_TOL[precision] and el <= GOLDEN_LAST_TOL[precision], (er, el)
    assert torch.equal(got.rollout[0], got.rollout[1])


# ---- vtq_k_rollout_step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
def test_step_kernel_masks_and_stays_in_bounds(fmt):
    """Three packed sequences of S = 37 with NaN canary rows behind the last one, a random positive r summing to 1: the output is finite,
    nothing past it is written, and it is 1/2 r + 1/2 mean_h r^T softmax of the planes' own Q / K in fp64.  An error eps per probability
    gives at most eps per output (sum r = 1): the bound is PROBS_TOL of test_probs_kernel_masks_and_stays_in_bounds.
    The key mask itself is pinned at every seam length, on keys that dominate, in tests/test_gpu_attention_seams.py."""
    lib = _lib.load()
    nseq, S, H = 3, 37, 768
    rows = nseq * S
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(rows + 64, 3 * H, generator=g) * 0.5
    three = fmt.endswith("x3")
    scale = 0.125 * math.log2(math.e) if three else 1.0
    qkv[:, :H] *= scale
    qkv[rows:] = float("nan")
    planes = to_planes(qkv.to(DEV), fmt)
    r = torch.rand(nseq, S, generator=g) + 0.05
    r = (r / r.sum(-1, keepdim=True)).float().to(DEV)
    n = nseq * S
    out = torch.full((n + 64,), float("nan"), device=DEV)
    part = torch.full((nseq * 12 * 1 * S + 64,), float("nan"), device=DEV)
    _lib.check(lib.vtq_k_rollout_step(planes.data_ptr(), planes[0].numel(), r.data_ptr(), out.data_ptr(), part.data_ptr(), nseq, S, S, H,
                                      _lib.NUM[fmt], int(three), stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[n:]).all() and torch.isnan(part[nseq * 12 * S:]).all(), "an element past an output was written"
    got = out[:n].view(nseq, S).double()
    assert torch.isfinite(got).all()
    v = planes[0].double() + (planes[1].double() if planes.shape[0] == 2 else 0)
    q = v[:rows, :H].view(nseq, S, 12, 64).permute(0, 2, 1, 3) / scale
    k = v[:rows, H:2 * H].view(nseq, S, 12, 64).permute(0, 2, 1, 3)
    P = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    ref = 0.5 * r.double() + 0.5 * torch.einsum("si,shij->sj", r.double(), P) / 12
    err = float((got - ref).abs().max())
    print(f"measured step kernel {fmt}: {err:.2e}")
    assert err <= PROBS_TOL[three]


# ---- footprint of the caller's outputs --------------------------------------------------------------------------------------
def test_outputs_keep_to_the_headers_extents():
    """rollout_out and last_attention_out carved at exactly 2 B S and 2 B h S floats inside guards (tests/footprint.py): no guard byte
    changes under either fill, the outputs are bit-identical across the fills and equal to the model's call; a NULL last_attention_out
    is accepted and gives the same rollout."""
    m, inp = stress_case("fp16x3")
    (pr, pd), (qr, qd), _ = inp
    B, N, S, h = 2, 130, 132, 12
    with torch.no_grad():
        q_ref, ref = m.forward_rollout(*inp)
    torch.cuda.synchronize()
    specs = [((B,), torch.float32), ((2, B, S), torch.float32), ((2, B, h, S), torch.float32), ((2, B, S), torch.float32)]
    a = Arena(fp.arena_bytes(specs), DEV)
    q = a.carve("q", (B,), torch.float32)
    roll = a.carve("rollout", (2, B, S), torch.float32)
    last = a.carve("last_attention", (2, B, h, S), torch.float32)
    roll2 = a.carve("rollout (null last_attention)", (2, B, S), torch.float32)
    lib, eng = m._engine_lib(), m._engine
    args = (pr.data_ptr(), pd.data_ptr(), qr.data_ptr(), qd.data_ptr(), None, None, B, N)

    def launch():
        _lib.check(lib.vtq_forward_rollout(eng, *args, q.data_ptr(), roll.data_ptr(), last.data_ptr(), stream()))
        _lib.check(lib.vtq_forward_rollout(eng, *args, q.data_ptr(), roll2.data_ptr(), None, stream()))

    def prepare():
        for t in (q, roll, last, roll2):
            t.zero_()
    gq, gr, gl, gr2 = a.run_twice(launch, lambda: [q, roll, last, roll2], prepare=prepare)
    bits = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(bits(gq), bits(q_ref)) and torch.equal(bits(gr), bits(ref.rollout)) and torch.equal(bits(gl), bits(ref.last_attention))
    assert torch.equal(bits(gr2), bits(gr))


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_train_mode_and_the_fp8_model_are_refused():
    m, inp = stress_case("fp16x3")
    m.train()
    with pytest.raises(NotImplementedError):
        m.forward_rollout(*inp)
    m.eval()
    m._FP8_EXPERIMENT = True
    with pytest.raises(NotImplementedError):
        m.forward_rollout(*inp)


def test_out_of_range_position_raises_and_the_next_call_succeeds():
    spec = VTAMIQ(**STRESS_KW, precision="fp16x3").spec
    m = build(STRESS_KW, stress_state(spec, 21, qk=5.0), "auto")               # the error word is read after every call
    (pr, pd), (qr, qd), _ = stress_case("fp16x3")[1]
    bad = qr.clone()
    bad[0, 3, 1] = 1.0
    with torch.no_grad():
        with pytest.raises(IndexError):
            m.forward_rollout((pr, pd), (bad, qd), None)
        _, got = m.forward_rollout((pr, pd), (qr, qd), None)
    check("after IndexError", "fp16x3", got, stress_reference("fp16x3"))


def test_a_set_token_trace_is_rejected_with_a_message_and_no_launch():
    m, inp = stress_case("fp16x3")
    (pr, pd), (qr, qd), _ = inp
    with torch.no_grad():
        m.forward_rollout(*inp)                                                 # creates the engine
    lib, eng = m._engine_lib(), m._engine
    B, N, S = 2, 130, 132
    trace = torch.zeros(4, 2 * B, 2, 768, device=DEV)
    q = torch.full((B,), 7.0, device=DEV)
    roll = torch.full((2, B, S), 7.0, device=DEV)
    _lib.check(lib.vtq_set_token_trace(eng, trace.data_ptr()))
    try:
        rc = lib.vtq_forward_rollout(eng, pr.data_ptr(), pd.data_ptr(), qr.data_ptr(), qd.data_ptr(), None, None, B, N, q.data_ptr(), roll.data_ptr(), None, stream())
    finally:
        lib.vtq_set_token_trace(eng, None)
    torch.cuda.synchronize()
    assert rc != 0 and b"token trace" in lib.vtq_last_error()
    assert bool((q == 7.0).all()) and bool((roll == 7.0).all()) and bool((trace == 0).all())
