"""forward_varlen on the GPU: B pairs with different patch counts in one launch sequence.

The contract every test here turns on: the score of pair b has the BITS the model gives for that pair alone (B = 1, N = lengths[b]), and each
sequence's attention rows have the bits vtq_k_attention gives that sequence alone.  The fp64 / oracle comparisons beside the bit checks keep
them from being vacuous (two equal wrong answers)."""
import ctypes as C
import functools
import json
import warnings

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests.footprint import FootprintError
from tests.gpu_util import elt_dtype, num_code, planes_of, planes_value, stream, to_planes
from tests.helpers import rel_err
from tests.test_gpu_footprint import Layout
from tests.test_gpu_kernels import ATTN_TOL, _attention_ref, _randn
from tests.test_gpu_parity import TOL, gate
from vtamiq_amd import VTAMIQ, _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
ATTN_LENGTHS = [9, 64, 65, 129, 128, 257, 63]
E2E_LENGTHS = [8, 63, 64, 127, 200, 77, 130, 56]        # ViT-B/16 without register tokens: S = 9, 64, 65, 128, 201, 78, 131, 57
bits16 = lambda t: t.contiguous().view(torch.int16)
bits32 = lambda t: t.contiguous().view(torch.int32)


# ---- 1, 2: the attention kernel ------------------------------------------------------------------------------------------
def _vl_attention(lib, P, out, lengths, H, fmt):
    rows = P.shape[1]
    arr = (C.c_int32 * len(lengths))(*lengths)
    _lib.check(lib.vtq_vl_attention(P.data_ptr(), rows * 3 * H, out.data_ptr(), rows * H, len(lengths), arr, H, num_code(fmt), stream()))


def _single(lib, P, out, row0, S, H, fmt):
    """vtq_k_attention on ONE sequence of the packed planes: nseq = 1, S = S_pad = S, pointers moved to its first row (same plane strides)."""
    rows = P.shape[1]
    _lib.check(lib.vtq_k_attention(P.data_ptr() + row0 * 3 * H * 2, rows * 3 * H, out.data_ptr() + row0 * H * 2, rows * H, 1, S, S, H,
                                   num_code(fmt), stream()))


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
@pytest.mark.parametrize("order", ["long_middle", "reversed"])
def test_attention_rows_have_the_bits_of_the_sequence_alone(fmt, order):
    lib = _lib.load()
    H = 768
    lengths = ATTN_LENGTHS if order == "long_middle" else ATTN_LENGTHS[::-1]
    R = sum(lengths)
    rows = R + 128
    qkv = _randn(rows, 3 * H, seed=16, scale=1.5)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    for r0, S in zip(starts, lengths):                    # the running maximum moves late in every sequence (online-softmax rescale path)
        qkv[r0 + S - 3, H:H + 64] *= 6.0
    P = to_planes(qkv, fmt, "a")
    npl = P.shape[0]
    out = torch.zeros((npl, rows, H), dtype=elt_dtype(fmt), device=DEV)
    _vl_attention(lib, P, out, lengths, H, fmt)
    alone = torch.zeros_like(out)
    for r0, S in zip(starts, lengths):
        _single(lib, P, alone, r0, S, H, fmt)
    torch.cuda.synchronize()
    assert torch.equal(bits16(out[:, :R]), bits16(alone[:, :R]))
    assert not bool(out[:, R:].any())                      # nothing stored at or behind row R
    val = planes_value(P)
    for r0, S in zip(starts, lengths):
        ref = _attention_ref(val[r0:r0 + S], 1, S, S, H)[0]
        err = (planes_value(out[:, r0:r0 + S]) - ref).abs().max().item() / ref.abs().max().item()
        assert err < ATTN_TOL[fmt], (fmt, r0, S, err)


@pytest.mark.parametrize("fmt", ["fp16x3", "fp16", "bf16x3"])
def test_attention_is_not_reached_by_nan_rows_of_another_sequence(fmt):
    """The variable-length twin of test_attention_is_not_reached_by_nan_rows_of_the_next_sequence: one middle sequence all NaN, the slack rows
    behind the last sequence inf -- every other sequence keeps its bits and stays finite."""
    lib = _lib.load()
    H = 768
    for lengths in (ATTN_LENGTHS, ATTN_LENGTHS[::-1]):
        R = sum(lengths)
        rows = R + 128
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        P = to_planes(_randn(rows, 3 * H, seed=41, scale=1.5), fmt, "a")
        clean = torch.zeros((P.shape[0], rows, H), dtype=elt_dtype(fmt), device=DEV)
        _vl_attention(lib, P, clean, lengths, H, fmt)
        k = len(lengths) // 2
        Pb = P.clone()
        Pb[:, starts[k]:starts[k] + lengths[k]] = float("nan")
        Pb[:, R:] = float("inf")
        dirty = torch.zeros_like(clean)
        _vl_attention(lib, Pb, dirty, lengths, H, fmt)
        torch.cuda.synchronize()
        for j, (r0, S) in enumerate(zip(starts, lengths)):
            a, b = clean[:, r0:r0 + S], dirty[:, r0:r0 + S]
            if j == k:
                assert bool(torch.isnan(b.float()).all())
            else:
                assert torch.equal(bits16(a), bits16(b)), (lengths, j)
                assert bool(torch.isfinite(b.float()).all())


# ---- 3: end to end -------------------------------------------------------------------------------------------------------
CONFIGS = {
    "plain": (dict(variant="ViT-B16"), 0, E2E_LENGTHS),
    "tokens8_layerscale": (dict(variant="ViT-B16", num_extra_tokens=8, use_layer_scale=True), 0, E2E_LENGTHS),
    "scales3": (dict(variant="ViT-B16", num_scales=3), 0, E2E_LENGTHS),
    "full_last_layer": (dict(variant="ViT-B16"), _lib.OPT_FULL_LAST_LAYER, E2E_LENGTHS),
    "vit_l16": (dict(variant="ViT-L16"), 0, [8, 130, 63]),
    "adapters": (dict(variant="ViT-B16", num_adapters=1), 0, E2E_LENGTHS),
}


def _kw(vit):
    return dict(vit_config=dict(num_keep_layers=2, pretrained=False, **vit), num_rgs=2, num_rcabs=2, ca_reduction=16)


def _model(vit, precision, options=0, seed=71):
    m = VTAMIQ(**json.loads(json.dumps(_kw(vit))), precision=precision, engine_options=options)
    sd = synth.make_state_dict(m.spec, seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval(), sd


def _pairs(spec, lengths, seed=300):
    """Per-pair CPU tensors: [(patches_ref, patches_dist), (pos_ref, pos_dist), (scales_ref, scales_dist) | (None, None)] with a batch axis of 1."""
    out = []
    for b, n in enumerate(lengths):
        pa, po, sc = synth.make_inputs(spec, 1, n, seed + b, aligned=bool(b & 1))
        t = lambda a: None if a is None else (torch.from_numpy(a[:, 0]).float(), torch.from_numpy(a[:, 1]).float())
        out.append((t(pa), t(po), t(sc) if sc is not None else (None, None)))
    return out


def _cat(pairs, device=DEV):
    """The concatenated (ref, dist) tensors forward_varlen takes."""
    cat = lambda k, i: None if pairs[0][k][i] is None else torch.cat([p[k][i][0] for p in pairs]).to(device)
    return tuple((cat(k, 0), cat(k, 1)) for k in range(3))


@functools.lru_cache(maxsize=None)
def _oracle_scores(name):
    """The reference forward (oracle, on the host) of every pair on its own: once per configuration, shared by the precisions."""
    vit, _, lengths = CONFIGS[name]
    m = VTAMIQ(**json.loads(json.dumps(_kw(vit))), precision="bf16")
    sd = synth.make_state_dict(m.spec, 71)
    return np.array([float(O.vtamiq_forward(O.to_torch(sd), m.spec, p, ps, sc)[0][0]) for p, ps, sc in _pairs(m.spec, lengths)])


def _e2e(name, precision):
    vit, options, lengths = CONFIGS[name]
    m, _ = _model(vit, precision, options)
    pairs = _pairs(m.spec, lengths)
    dev = lambda ts: tuple(None if t is None else t.to(DEV) for t in ts)
    with torch.no_grad():
        p, ps, sc = _cat(pairs)
        q = m.forward_varlen(p, ps, sc, lengths)[0]
        alone = torch.cat([m(dev(a), dev(b), dev(c))[0] for a, b, c in pairs])
        again = m.forward_varlen(p, ps, sc, torch.tensor(lengths))[0]        # after the B = 1 calls: same tables, same bits
    assert q.shape == (len(lengths),) and q.dtype == torch.float32 and bool(torch.isfinite(q).all())
    assert torch.equal(bits32(q), bits32(alone)), (q - alone).abs().max().item()
    assert torch.equal(bits32(q), bits32(again))
    m.check_inputs()
    ref = _oracle_scores(name)
    e = rel_err(q.cpu().numpy(), ref)
    print(f"\n[varlen {name} {precision}] {e}")
    assert gate(q.cpu().numpy(), ref, TOL[precision]), e


@pytest.mark.parametrize("precision", ["fp16x3", "fp16x2", "bf16"])
@pytest.mark.parametrize("name", ["plain", "tokens8_layerscale", "scales3", "full_last_layer"])
def test_scores_have_the_bits_of_the_pair_alone(name, precision):
    _e2e(name, precision)


def test_scores_have_the_bits_of_the_pair_alone_vit_l16():
    _e2e("vit_l16", "fp16x3")


def test_scores_have_the_bits_of_the_pair_alone_adapters():
    """Adapters: the full last layer (no CLS-only tail) and two more GEMMs per residual branch, on rows addressed by the tables."""
    _e2e("adapters", "fp16x3")


# ---- 4: uniform lengths --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    return _model(dict(variant="ViT-B16"), "fp16x3")[0]


def test_equal_lengths_are_forward(plain):
    m = plain
    B, N = 5, 77
    pa, po, _ = synth.make_inputs(m.spec, B, N, 12, aligned=False)
    pr, pd = (torch.from_numpy(pa[:, i]).to(DEV) for i in (0, 1))
    qr, qd = (torch.from_numpy(po[:, i]).to(DEV) for i in (0, 1))
    with torch.no_grad():
        q = m((pr, pd), (qr, qd), (None, None))[0]
        v = m.forward_varlen((pr.flatten(0, 1), pd.flatten(0, 1)), (qr.flatten(0, 1), qd.flatten(0, 1)), (None, None), [N] * B)[0]
    assert torch.equal(bits32(q), bits32(v))


def test_permuted_pairs_permute_the_bits_and_lists_equal_tensors(plain):
    m = plain
    lengths = E2E_LENGTHS
    pairs = _pairs(m.spec, lengths, seed=500)
    perm = [3, 0, 7, 5, 1, 6, 2, 4]
    with torch.no_grad():
        q = m.forward_varlen(*_cat(pairs), lengths)[0]
        qp = m.forward_varlen(*_cat([pairs[i] for i in perm]), [lengths[i] for i in perm])[0]
        as_list = lambda k, i: [p[k][i][0].to(DEV) for p in pairs]
        ql = m.forward_varlen((as_list(0, 0), as_list(0, 1)), (as_list(1, 0), as_list(1, 1)), (None, None), lengths)[0]
    assert torch.equal(bits32(qp), bits32(q[perm]))
    assert torch.equal(bits32(ql), bits32(q))


# ---- 5: input policy -----------------------------------------------------------------------------------------------------
def test_input_policy(plain):
    m = plain
    lengths = E2E_LENGTHS
    pairs = _pairs(m.spec, lengths, seed=600)
    p, ps, sc = _cat(pairs)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    with torch.no_grad():
        q = m.forward_varlen(p, ps, sc, lengths)[0]
        m.check_inputs()
        bad_pos = (ps[0].clone(), ps[1])
        bad_pos[0][starts[3] + 5, 1] = 1.5
        m.forward_varlen(p, bad_pos, sc, lengths)
        with pytest.raises(IndexError):
            m.check_inputs()
        bad_p = (p[0], p[1].clone())
        bad_p[1][starts[3]:starts[3] + lengths[3]] = float("nan")
        qn = m.forward_varlen(bad_p, ps, sc, lengths)[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
    keep = [b for b in range(len(lengths)) if b != 3]
    assert bool(torch.isnan(qn[3])) and torch.equal(bits32(qn[keep]), bits32(q[keep]))
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_varlen(p, ps, sc, lengths[:-1] + [lengths[-1] + 1])
    with pytest.raises(ValueError, match="CUDA"):
        m.forward_varlen(p, ps, sc, torch.tensor(lengths, device=DEV))
    with pytest.raises(ValueError, match="lengths"):
        m.forward_varlen(p, ps, sc, lengths[:-1] + [0])


def test_auto_precision_gives_nan_only_where_the_reference_would():
    """precision="auto" as in forward(): NaN patches in pair 1 -> its score is NaN, the others keep the bits of the clean call, the model
    stays in fp16x3; a position outside [0, 1) raises IndexError from the call itself."""
    m, _ = _model(dict(variant="ViT-B16"), "auto")
    lengths = [8, 63, 64]
    pairs = _pairs(m.spec, lengths, seed=700)
    p, ps, sc = _cat(pairs)
    with torch.no_grad():
        q = m.forward_varlen(p, ps, sc, lengths)[0]
        bad_p = (p[0].clone(), p[1])
        bad_p[0][8:8 + 63] = float("nan")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            qn = m.forward_varlen(bad_p, ps, sc, lengths)[0]
        assert any("non-finite" in str(x.message) for x in w)
        assert m.engine_precision == "fp16x3"
        assert bool(torch.isnan(qn[1])) and torch.equal(bits32(qn[[0, 2]]), bits32(q[[0, 2]]))
        bad_pos = (ps[0], ps[1].clone())
        bad_pos[1][70, 0] = -0.25
        with pytest.raises(IndexError):
            m.forward_varlen(p, bad_pos, sc, lengths)


# ---- 6: streams and workspace regrowth -----------------------------------------------------------------------------------
def test_side_stream_and_regrowth(plain):
    m = plain
    lengths = E2E_LENGTHS
    pairs = _pairs(m.spec, lengths, seed=800)
    small = [pairs[0], pairs[1]]
    with torch.no_grad():
        fresh, _ = _model(dict(variant="ViT-B16"), "fp16x3")
        q_fresh = fresh.forward_varlen(*_cat(pairs), lengths)[0]             # first call of a new engine: the large batch
        grown, _ = _model(dict(variant="ViT-B16"), "fp16x3")
        grown.forward_varlen(*_cat(small), lengths[:2])                      # a small batch first ...
        q_grown = grown.forward_varlen(*_cat(pairs), lengths)[0]             # ... then the workspace grows
        q_default = m.forward_varlen(*_cat(pairs), lengths)[0]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        args = _cat(pairs)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            q_side = m.forward_varlen(*args, lengths)[0]
            q_side2 = m.forward_varlen(*_cat(small), lengths[:2])[0]         # back to back on the side stream: the tables are re-uploaded
        side.synchronize()
    assert torch.equal(bits32(q_grown), bits32(q_fresh)) and torch.equal(bits32(q_default), bits32(q_fresh))
    assert torch.equal(bits32(q_side), bits32(q_fresh))
    assert torch.equal(bits32(q_side2), bits32(q_fresh[:2]))


# ---- 7: footprint --------------------------------------------------------------------------------------------------------
def test_forward_varlen_keeps_to_the_callers_tensors():
    m, _ = _model(dict(variant="ViT-B16", num_scales=3), "fp16x3")
    lengths = [8, 63, 64, 45]
    total = sum(lengths)
    (pr, pd), (qr, qd), (sr, sd) = _cat(_pairs(m.spec, lengths, seed=900))
    with torch.no_grad():
        q_ref = m.forward_varlen((pr, pd), (qr, qd), (sr, sd), lengths)[0]    # the ordinary call (it also creates the engine)
    torch.cuda.synchronize()
    L = Layout()
    for i in range(2):
        L.add(f"patches{i}", (total, 3, 16, 16), F32, 16 * 4), L.add(f"pos{i}", (total, 2), F32), L.add(f"scales{i}", (total,), F32)
    L.add("q", (len(lengths),), F32)
    a, v = L.build()
    for i, (pt, po, sc) in enumerate(((pr, qr, sr), (pd, qd, sd))):
        v[f"patches{i}"].copy_(pt), v[f"pos{i}"].copy_(po), v[f"scales{i}"].copy_(sc)
    lib, eng = m._engine_lib(), m._engine
    p = lambda n: v[n].data_ptr()
    arr = (C.c_int32 * len(lengths))(*lengths)
    (got,) = a.run_twice(lambda: _lib.check(lib.vtq_forward_varlen(eng, p("patches0"), p("patches1"), p("pos0"), p("pos1"), p("scales0"), p("scales1"),
                                                                   len(lengths), arr, p("q"), stream())),
                         lambda: [v["q"]], prepare=lambda: v["q"].zero_())
    assert bool(torch.isfinite(got).all()) and torch.equal(bits32(got), bits32(q_ref))
    flags = C.c_int32(-1)
    _lib.check(lib.vtq_input_errors(eng, C.byref(flags), stream()))
    assert flags.value == 0


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
def test_vl_attention_keeps_to_the_extents_of_the_header(fmt):
    """qkv has exactly R + 127 rows (the header: "up to 127 rows behind row R are read"), the last 127 "value irrelevant"; out exactly R rows.
    Last sequence 129 and 257 rows: one row past a 128-row query block, where the over-read is largest; and 9 rows."""
    lib = _lib.load()
    dt, npl, H = elt_dtype(fmt), planes_of(fmt, "a"), 768
    for lengths in ([64, 9, 129], [65, 257], [130, 9]):
        R = sum(lengths)
        rows_in = R + 127
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        qkv = _randn(rows_in, 3 * H, seed=16, scale=1.5)
        for r0, S in zip(starts, lengths):
            qkv[r0 + S - 3, H:H + 64] *= 6.0
        P = to_planes(qkv, fmt, "a")
        L = Layout()
        L.add("qkv", (npl, rows_in, 3 * H), dt, 3 * H * 2, rows_in * 3 * H * 2)
        L.add("out", (npl, R, H), dt, H * 2, R * H * 2)
        a, v = L.build()
        v["qkv"].copy_(P)
        a.scratch("qkv", "rows behind the last sequence", R * 3 * H * 2, 127 * 3 * H * 2, rows_in * 3 * H * 2, npl)
        arr = (C.c_int32 * len(lengths))(*lengths)
        try:
            (got,) = a.run_twice(lambda: _lib.check(lib.vtq_vl_attention(v["qkv"].data_ptr(), rows_in * 3 * H, v["out"].data_ptr(), R * H, len(lengths),
                                                                         arr, H, num_code(fmt), stream())),
                                 lambda: [v["out"]], prepare=lambda: v["out"].zero_())
        except FootprintError as e:
            raise AssertionError(f"{fmt} lengths={lengths}: {e}") from e
        val = planes_value(P)
        for r0, S in zip(starts, lengths):
            ref = _attention_ref(val[r0:r0 + S], 1, S, S, H)[0]
            err = (planes_value(got[:, r0:r0 + S]) - ref).abs().max().item() / ref.abs().max().item()
            assert err < ATTN_TOL[fmt], (fmt, lengths, r0, err)
