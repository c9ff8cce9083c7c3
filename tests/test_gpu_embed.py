"""The embedding front end, row by row, at position and scale edges.

pack_patches_kernel, embed_index_kernel, embed_rows_kernel, tokens_kernel, zero_pad_rows_kernel (elementwise.hip) and the EPI_EMBED epilogue
of the patch GEMM (gemm.hip, gemm_st.hip) have no kernel entry of their own.  They are observed through vtq_debug_stop_after(engine, 0):
stage 0 (LayerNorm 1 of layer 0) only writes lnbuf, so `x` of vtq_debug_buffers then holds the embedding output of the entry call that was
made (tests/stage_probe.py StageProbe with `call`).  Every row of x -- token rows, patch rows and the pad rows up to M_pad + 128 -- is
compared with oracle.embeddings of each sequence alone at its packed row, for positions on and next to every cell border of the positional
table (tests/embed_probe.py; tests/test_embed_cases.py proves the case builder on the host).

  * pre-embedded input: bit-equal to fp32 torch, (feat + pos_row) + scale_row;
  * patch input, zero patch weights: every patch row IS pos_table[idx] (+ scale_table[sidx]): the table index, exactly, in every numerics
    mode and tile shape;
  * patch input, random weights: per-row error against fp64 within STAGE_BOUND[mode]["embed"] of tests/test_gpu_stages.py;
  * through every entry and addressing mode; out-of-range positions, NaN scale ids, fp64 / fp16 inputs; and the check failing on purpose.
"""
import json

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests import embed_probe as ep
from tests.stage_probe import RefWeights, StageProbe, row_error
from tests.test_gpu_stages import STAGE_BOUND
from vtamiq_amd import VTAMIQ, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_MODES = ["fp16x3", "bf16x3", "fp16x2", "fp16", "bf16"]
# vtq_debug_gemm_variant (kernels.h GEMM_TILE_256, GEMM_ST_64, GEMM_ST_64X2, GEMM_ST_128): the persistent 256 x 256 kernel, 64 x 64 tiles with an
# operand ring of 3 and of 2, 128 x 128 tiles (its own wave layout, so its own EPI_EMBED gather / scatter)
TILE_SHAPES = (0, 1, 2, 3)


def build(mkey, precision, zero_patch=False):
    m = VTAMIQ(**json.loads(json.dumps(ep.MODELS[mkey])), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ep.state_dict(mkey, zero_patch).items()}, strict=True)
    return m.to(DEV).eval()


_w = {}


def weights(mkey, zero_patch=False):
    """The model's weights as fp32 CPU torch tensors: computed once, never modified."""
    key = (mkey, zero_patch)
    if key not in _w:
        _w[key] = O.to_torch(ep.state_dict(mkey, zero_patch))
    return _w[key]


def front_end(model, call, d):
    """-> (x, flags): the residual stream behind the embedding front end of one entry call, rows [0, M_pad + 128) on the CPU, and the
    vtq_input_errors word of the same call run to its end (the stopped forward's scores and flags are discarded)."""
    T = model.spec.num_tokens
    rows = call.token_rows(T)
    pr = StageProbe(model, None, 1, rows - T, nimg=1, call=lambda: ep.run(model, call, d))      # one whole call: engine, workspace, flags
    flags = model._read_flags()
    x = pr.grab_stop(0, want=("x",))["x"].cpu()               # (the hook is reset in grab_stop's finally)
    model._read_flags()
    return x, flags


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_rows(x, want, tag):
    """Every sequence row has the expected values and every row behind them, up to M_pad + 128, is zero."""
    n = want.shape[0]
    bad = ep.bad_rows(x[:n], want)
    assert not bad, f"{tag}: {len(bad)} of {n} rows differ from the reference, first {bad[:8]}"
    pad = torch.nonzero((bits(x[n:]) != 0).any(-1)).flatten().tolist()
    assert not pad, f"{tag}: pad rows {[n + r for r in pad[:8]]} of [{n}, {x.shape[0]}) are not zero"


def case(mkey, call, seed, tokens_in, zero_patch=False):
    spec = ep.spec_of(mkey)
    inp = ep.make_inputs(spec, call, seed, tokens_in)
    return spec, inp, ep.to_device(call, inp, DEV), ep.expected(weights(mkey, zero_patch), spec, call, inp)


# ---- 1 / 5: pre-embedded input through every entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkey", ["b16_t1", "b16_t3_s2"])
@pytest.mark.parametrize("entry", [e for e in ep.ENTRY_CALLS if e != "varlen"])       # forward_varlen offers no pre-embedded input
def test_pre_embedded_rows_are_bit_equal(entry, mkey):
    call = ep.ENTRY_CALLS[entry]
    spec, inp, d, want = case(mkey, call, 31, tokens_in=True)
    model = build(mkey, "fp16x3")
    x, flags = front_end(model, call, d)
    assert flags == 0, f"false alarm {flags} on in-range positions and clamped scale ids"
    assert_rows(x, want, f"{entry} {mkey}")
    # stated on their own: token row 0 = cls + pos_table[0], the register rows are copies
    w, T = weights(mkey), spec.num_tokens
    e = "transformer.embeddings."
    row = 0
    for n in call.seq_lengths():
        assert torch.equal(x[row], w[e + "cls_token"][0, 0] + w[e + "positional_embeddings.positional_embeddings"][0, 0])
        if T > 1:
            assert torch.equal(bits(x[row + 1:row + T]), bits(w[e + "extra_tokens"][0]))
        row += n + T
    # a larger call whose every feature is NaN leaves NaN in every row it wrote; the same call behind it has the same rows and zero pad rows
    big = ep.Call("forward", (2, 2), 400)
    binp = ep.make_inputs(spec, big, 32, tokens_in=True)
    binp["p"][:] = np.nan
    ep.run(model, big, ep.to_device(big, binp, DEV))
    assert model._read_flags() & 2
    x2, flags2 = front_end(model, call, d)
    assert flags2 == 0
    assert_rows(x2, want, f"{entry} {mkey} behind a NaN call")


# ---- 2 / 5: patch input, the table index exactly, every mode, entry and tile shape --------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES)
def test_patch_rows_hold_the_indexed_table_rows(mode):
    lib = _lib.load()
    for mkey in ("b16_t1", "b16_t3_s2"):
        model = build(mkey, mode, zero_patch=True)
        for entry, call in ep.ENTRY_CALLS.items():
            spec, inp, d, want = case(mkey, call, 41, tokens_in=False, zero_patch=True)
            xs = []
            for shape in TILE_SHAPES:
                try:
                    _lib.check(lib.vtq_debug_gemm_variant(shape))
                    x, flags = front_end(model, call, d)
                finally:
                    _lib.check(lib.vtq_debug_gemm_variant(-1))
                assert flags == 0, (entry, mkey, shape, flags)
                assert_rows(x, want, f"{entry} {mkey} {mode} tile shape {shape}")
                xs.append(x)
            assert all(torch.equal(bits(xs[0]), bits(v)) for v in xs[1:]), f"{entry} {mkey} {mode}: x differs between the tile shapes"


# ---- 3 / 4: shapes; exact index and per-row numerics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkey,shape", ep.SHAPE_CASES)
def test_shapes_index_exactly(mkey, shape):
    call = ep.SHAPE_CALLS[shape]
    model = build(mkey, "fp16x3", zero_patch=True)
    for tokens_in in (False, True):
        spec, inp, d, want = case(mkey, call, 51, tokens_in, zero_patch=True)
        x, flags = front_end(model, call, d)
        assert flags == 0
        assert_rows(x, want, f"{mkey} {shape} {'pre-embedded' if tokens_in else 'patches'}")


@pytest.mark.parametrize("mkey,shape", ep.SHAPE_CASES)
def test_shapes_numerics_per_row(mkey, shape):
    """Random patch weights: every row against fp64 of the model's own fp32 weights through tests/stage_probe.py RefWeights (positions and
    scale ids stay fp32: the index is the reference's), error per row as stage_probe.row_error measures it, bound STAGE_BOUND[mode]["embed"]
    as tests/test_gpu_stages.py set it.  The reference is evaluated on the HOST (RefWeights(device="cpu")), where test_gpu_stages.py evaluates
    it on the GPU: these shapes are small, and the comparison then uses no GPU arithmetic at all."""
    call = ep.SHAPE_CALLS[shape]
    spec = ep.spec_of(mkey)
    inp = ep.make_inputs(spec, call, 61, tokens_in=False)
    d = ep.to_device(call, inp, DEV)
    ref = ep.expected(RefWeights(ep.state_dict(mkey), device="cpu"), spec, call, inp, dtype=torch.float64)
    n, over = ref.shape[0], []
    for mode in ALL_MODES:
        x, flags = front_end(build(mkey, mode), call, d)
        assert flags == 0
        err, col = row_error(x[:n], ref)
        r = int(torch.argmax(err))
        worst, bound = float(err[r]), STAGE_BOUND[mode]["embed"]
        print(f"   [embed {mkey} {shape} {mode}] {n} rows, worst row {worst:.2e} at (row {r}, column {int(col[r])})   bound {bound:.2g}"
              f"{'' if worst <= bound else '   <-- OVER'}")
        if not worst <= bound:
            over.append((mode, r, worst, bound))
        assert not (bits(x[n:]) != 0).any(), f"{mkey} {shape} {mode}: pad rows behind row {n} are not zero"
    assert not over, over


# ---- 6: out-of-range positions ---------------------------------------------------------------------------------------------------------------
OOR_MODEL, OOR_CALL, OOR_ROW = "b16_t3_s2", ep.Call("forward", (2, 2), 24), 37


@pytest.fixture(scope="module")
def oor_shared():
    """The clean call of the out-of-range tests: its inputs, its reference rows, its rows on an engine that ran nothing else, and the two
    engines the tests share: one explicit-precision model and one drop-in "auto" model."""
    spec, inp, d, want = case(OOR_MODEL, OOR_CALL, 71, tokens_in=False, zero_patch=True)
    x, flags = front_end(build(OOR_MODEL, "fp16x3", zero_patch=True), OOR_CALL, d)
    assert flags == 0
    assert_rows(x, want, "clean call, fresh engine")
    return dict(spec=spec, inp=inp, d=d, want=want, fresh=x, model=build(OOR_MODEL, "fp16x3", zero_patch=True),
                auto=build(OOR_MODEL, "auto", zero_patch=True))


@pytest.fixture
def oor(oor_shared):
    """oor_shared with nothing pending on its engines: a test that failed between a flagged call and the clean call behind it leaves its
    error word for nobody (vtq_input_errors clears on read; the debug stop is reset in StageProbe's finally)."""
    for m in (oor_shared["model"], oor_shared["auto"]):
        if m._engine is not None:
            m._read_flags()
    return oor_shared


def table_rows(spec, pidx, sidx):
    w, e = weights(OOR_MODEL, zero_patch=True), "transformer.embeddings."
    return (0.0 + w[e + "positional_embeddings.positional_embeddings"][0, pidx]) + w[e + "scale_embeddings.scale_embeddings"][0, sidx]


def check_flagged(s, inp_bad, want_row, tag):
    """One offending input row: bit 0 and not bit 1; the row holds want_row; every other row has the clean call's bits; the drop-in model
    raises IndexError; the next clean call reports nothing and has a fresh engine's bits."""
    spec, model, T = s["spec"], s["model"], s["spec"].num_tokens
    dbad = ep.to_device(OOR_CALL, inp_bad, DEV)
    x, flags = front_end(model, OOR_CALL, dbad)
    assert flags & 3 == 1, f"{tag}: vtq_input_errors {flags}, expected bit 0 alone"
    trow, n = ep.token_row_of_patch(OOR_CALL, T, OOR_ROW), s["want"].shape[0]
    assert torch.equal(x[trow], want_row), f"{tag}: row {trow} does not hold the clamped table row"
    keep = torch.arange(x.shape[0]) != trow
    assert torch.equal(bits(x[keep]), bits(s["fresh"][keep])), f"{tag}: rows other than {trow} moved"
    with pytest.raises(IndexError):
        ep.run(s["auto"], OOR_CALL, dbad)
    x2, flags2 = front_end(model, OOR_CALL, s["d"])
    assert flags2 == 0, f"{tag}: the next clean call reports {flags2}"
    assert torch.equal(bits(x2), bits(s["fresh"])), f"{tag}: the next clean call does not have a fresh engine's bits"
    assert ep.run(s["auto"], OOR_CALL, s["d"])[0].isfinite().all()          # and the drop-in model takes the clean call again


@pytest.mark.parametrize("name,value", ep.OUT_OF_RANGE, ids=[n for n, _ in ep.OUT_OF_RANGE])
def test_out_of_range_position_is_clamped_and_reported(name, value, oor):
    s = oor
    spec, G = s["spec"], s["spec"].pos_grid
    for coord in (0, 1):
        inp = dict(s["inp"], pos=s["inp"]["pos"].copy())
        inp["pos"][OOR_ROW, coord] = value
        cells = [int(c) for c in ep.cell(s["inp"]["pos"][OOR_ROW], G)]       # the other coordinate keeps its cell
        cells[coord] = ep.clamped_cell(value, G)
        sidx = int(O.scale_index(torch.from_numpy(inp["sc"][OOR_ROW:OOR_ROW + 1]), spec.num_scales))
        check_flagged(s, inp, table_rows(spec, cells[0] * G + cells[1] + 1, sidx), f"pos[{coord}] = {name}")


# ---- 7: NaN scale id ---------------------------------------------------------------------------------------------------------------------------
def test_nan_scale_id_is_reported(oor):
    """The reference's clamp keeps a NaN and its table lookup raises (tests/test_embed_cases.py): the engine takes scale-table row 1 and
    reports it through bit 0, as it does a NaN position.  Every other scale id, +-inf included, is the reference's clamp with no flag: the
    in-range tests above hold all of them and assert flags == 0."""
    s = oor
    spec, G = s["spec"], s["spec"].pos_grid
    inp = dict(s["inp"], sc=s["inp"]["sc"].copy())
    inp["sc"][OOR_ROW] = np.nan
    pidx = int(O.pos_index(torch.from_numpy(inp["pos"][OOR_ROW:OOR_ROW + 1]), G))
    check_flagged(s, inp, table_rows(spec, pidx, 1), "scale id NaN")


# ---- 8: input dtype ----------------------------------------------------------------------------------------------------------------------------
def test_positions_and_scales_of_other_dtypes_behave_as_their_fp32_cast(oor):
    """model.py casts every input to fp32 (the loader's contract, train.py:254-255) before the engine floors pos * G in fp32: a float64 position
    whose fp64 floor is another cell than its fp32 cast's floor takes the fp32 cell."""
    s = oor
    spec, G, model = s["spec"], s["spec"].pos_grid, s["model"]
    v = ep.edge_values(G)
    d32 = float(v[ep.differing(v, G)][0])                                    # an fp32 value: fp32 product rounds up to k, the exact one does not
    pos64 = s["inp"]["pos"].astype(np.float64)
    pos64[5, 0], pos64[6, 1] = d32, 0.5 - 1e-12                              # 0.5 - 1e-12: cell G / 2 - 1 in fp64, 0.5 -> cell G / 2 as fp32
    p64 = torch.from_numpy(pos64)
    assert (O.pos_index(p64, G) != O.pos_index(p64.float(), G))[[5, 6]].all()
    grid16 = np.concatenate([np.arange(G) / G, (np.arange(G) + 0.5) / G]).astype(np.float16)
    R = OOR_CALL.patch_rows()
    pos16 = np.stack([grid16[np.arange(R) % (2 * G)], grid16[(np.arange(R) * 7 + 1) % (2 * G)]], 1)
    assert float(pos16.max()) < 1.0
    for tag, pos, dt in (("float64", pos64, torch.float64), ("float16", pos16, torch.float16)):
        inp_dt = dict(s["inp"], pos=pos)
        d = ep.to_device(OOR_CALL, inp_dt, DEV, sc_dtype=dt)
        assert d["pos"][0].dtype == dt and d["sc"][0].dtype == dt
        as32 = dict(s["inp"], pos=pos.astype(np.float32), sc=torch.from_numpy(s["inp"]["sc"]).to(dt).float().numpy())
        want = ep.expected(weights(OOR_MODEL, zero_patch=True), spec, OOR_CALL, as32)
        x, flags = front_end(model, OOR_CALL, d)
        assert flags == 0, (tag, flags)
        assert_rows(x, want, f"{tag} positions and scale ids")


# ---- 9: the check can fail ---------------------------------------------------------------------------------------------------------------------
def test_the_check_reports_exactly_the_rows_that_are_wrong():
    mkey, call = "b16_t1", ep.ENTRY_CALLS["forward"]
    spec, inp, d, want = case(mkey, call, 41, tokens_in=False, zero_patch=True)
    G, T, w = spec.pos_grid, spec.num_tokens, weights(mkey, zero_patch=True)
    x, _ = front_end(build(mkey, "fp16x3", zero_patch=True), call, d)
    n = want.shape[0]
    assert ep.bad_rows(x[:n], want) == []
    # one position moved across a border, in the reference's copy only
    r = 150
    moved = dict(inp, pos=inp["pos"].copy())
    moved["pos"][r, 1] = (ep.cell(inp["pos"][r, 1:], G)[0] + 1) % G / G + 0.25 / G
    assert ep.bad_rows(x[:n], ep.expected(w, spec, call, moved)) == [ep.token_row_of_patch(call, T, r)]
    # the reference's index evaluated in fp64: exactly the rows the host proved to have another fp64 floor
    p = torch.from_numpy(inp["pos"])
    differ = torch.nonzero(O.pos_index(p, G) != O.pos_index(p.double(), G)).flatten().tolist()
    assert len(differ) >= 20
    got = ep.bad_rows(x[:n], ep.expected(w, spec, call, inp, pos_dtype=torch.float64))
    assert got == [ep.token_row_of_patch(call, T, q) for q in differ]
