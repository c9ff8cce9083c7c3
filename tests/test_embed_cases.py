"""What tests/test_gpu_embed.py relies on, checked on the host with oracle.pos_index / oracle.scale_index alone (tests/embed_probe.py): the
edge set holds every value in both coordinates, the four corners and (full) every table row; every index lies inside the table; and it holds
positions whose fp32 floor(pos * G) is not their fp64 floor.  They fail here, without a GPU, when someone edits the case builder."""
import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests import embed_probe as ep

F32 = np.float32


def _bits(a):
    return set(np.asarray(a, dtype=F32).view(np.uint32).tolist())          # by bit pattern: -0.0 and 0.0 are two values


@pytest.mark.parametrize("G", [24, 48])
def test_edge_values_are_the_listed_ones(G):
    v = ep.edge_values(G)
    assert v.dtype == F32 and len(v) == 4 * G + 4
    want = []
    for k in range(G):
        b = F32(k) / F32(G)
        want += [b, np.nextafter(b, F32(2)), (F32(k) + F32(0.5)) / F32(G)]
        if k >= 1:
            want.append(np.nextafter(b, F32(-1)))
    want += [F32(0.0), F32(-0.0), F32(1e-45), F32(1 - 1e-6), np.nextafter(F32(1), F32(0))]
    assert _bits(v) == _bits(want)
    assert F32(1e-45) > 0 and F32(1e-45) == np.nextafter(F32(0), F32(1))   # the smallest subnormal is one
    assert (v < 1).all() and (v >= 0).all()


@pytest.mark.parametrize("G", [24, 48])
def test_edge_rows_cover_both_coordinates_the_corners_and_the_table(G):
    v, rows = ep.edge_values(G), ep.edge_rows(G)
    assert _bits(rows[:, 0]) == _bits(v) and _bits(rows[:, 1]) == _bits(v)
    idx = O.pos_index(torch.from_numpy(rows), G)
    assert {1, G, G * (G - 1) + 1, G * G} <= set(idx.tolist())             # the four corner cells
    assert 1 <= int(idx.min()) and int(idx.max()) <= G * G
    full = np.concatenate([rows, ep.full_rows(G)])
    assert set(O.pos_index(torch.from_numpy(full), G).tolist()) == set(range(1, G * G + 1))


@pytest.mark.parametrize("G,below,total", [(24, 3, 10), (48, 8, 23)])
def test_edge_values_hold_differing_fp32_and_fp64_floors(G, below, total):
    """Just below k / G the fp32 product rounds up to k for some k (3 of 23 for G = 24, 8 of 47 for G = 48); a border k / G that was rounded
    down in fp32 has the same property.  In fp64 all of them land in cell k - 1."""
    v = ep.edge_values(G)
    d = ep.differing(v, G)
    assert int(ep.differing(v[:G - 1], G).sum()) == below and int(d.sum()) == total
    assert (ep.cell(v[d], G, torch.float32) == ep.cell(v[d], G, torch.float64) + 1).all()
    rows = torch.from_numpy(ep.edge_rows(G))
    assert int((O.pos_index(rows, G) != O.pos_index(rows.double(), G)).sum()) >= 2 * total


def test_every_gpu_case_holds_what_it_claims():
    for name, call in ep.ENTRY_CALLS.items():
        for mkey in ("b16_t1", "b16_t3_s2"):
            spec = ep.spec_of(mkey)
            G = spec.pos_grid
            inp = ep.make_inputs(spec, call, 11, tokens_in=False)
            e = np.concatenate([ep.edge_rows(G), ep.full_rows(G)]) if call.full else ep.edge_rows(G)
            assert call.patch_rows() >= len(e) and np.array_equal(inp["pos"][:len(e)].view(np.uint32), e.view(np.uint32)), name
            idx = O.pos_index(torch.from_numpy(inp["pos"]), G)
            assert 1 <= int(idx.min()) and int(idx.max()) <= G * G, name
            if inp["sc"] is not None:                          # every scale id, each checked against the reference's clamp
                assert _bits(inp["sc"]) == _bits(ep.scale_values(spec.num_scales)) and not np.isnan(inp["sc"]).any()
                sidx = O.scale_index(torch.from_numpy(inp["sc"]), spec.num_scales)
                assert 1 <= int(sidx.min()) and int(sidx.max()) <= spec.num_scales
    for mkey, shape in ep.SHAPE_CASES:
        spec, call = ep.spec_of(mkey), ep.SHAPE_CALLS[shape]
        G = spec.pos_grid
        inp = ep.make_inputs(spec, call, 11, tokens_in=False)
        idx = O.pos_index(torch.from_numpy(inp["pos"]), G)
        assert 1 <= int(idx.min()) and int(idx.max()) <= G * G
        if call.full:
            assert call.N >= G * G and set(idx.tolist()) == set(range(1, G * G + 1)), (mkey, shape)
    # the shapes: 2, 255, 256 and 257 packed patch rows, T = 1, 3 and 9, both grids, H = 1024, no / 2 / 3 scales, one full set per grid
    assert {ep.SHAPE_CALLS[s].patch_rows() for _, s in ep.SHAPE_CASES} >= {2, 255, 256, 257}
    specs = [ep.spec_of(m) for m, _ in ep.SHAPE_CASES]
    assert {s.num_tokens for s in specs} >= {1, 3, 9} and {s.pos_grid for s in specs} == {24, 48}
    assert {s.hidden_size for s in specs} == {768, 1024} and {s.num_scales for s in specs} == {0, 2, 3}
    assert {ep.spec_of(m).pos_grid for m, s in ep.SHAPE_CASES if ep.SHAPE_CALLS[s].full} == {24, 48}


def test_entry_calls_cover_every_addressing_mode():
    kinds = {c.kind for c in ep.ENTRY_CALLS.values()}
    assert kinds == {"forward", "pairwise", "vit", "group", "encode", "cached", "varlen"}
    groups = [c.images for c in ep.ENTRY_CALLS.values() if c.kind == "group"]
    assert (1, 5) in groups and (3, 2) in groups                           # R0 != BN both ways
    L = ep.VARLEN_LENGTHS
    pre = np.cumsum([0] + L)
    assert 1 in L and L.index(max(L)) not in (0, len(L) - 1)
    assert any(a < 256 < b for a, b in zip(pre, pre[1:]))                  # a pair's patch rows cross row 256
    call = ep.ENTRY_CALLS["varlen"]
    assert call.seq_lengths() == L + L and call.token_rows(3) == 2 * (sum(L) + 3 * len(L))
    assert ep.token_row_of_patch(call, 3, 0) == 3 and ep.token_row_of_patch(call, 3, 1) == 4 + 3
    assert ep.token_row_of_patch(call, 3, sum(L)) == sum(L) + 3 * len(L) + 3


def test_out_of_range_positions_leave_the_table_in_the_reference():
    """Each out-of-range value has floor(v * G) outside [0, G) or NaN in fp32; clamped_cell restates the kernel's clamp."""
    for G in (24, 48):
        for name, v in ep.OUT_OF_RANGE:
            f = torch.floor(torch.tensor(v, dtype=torch.float32) * G)
            assert not bool((f >= 0) & (f < G)), name
            assert ep.clamped_cell(v, G) == (G - 1 if v >= 1 else 0), name
    f = torch.floor(torch.tensor(dict(ep.OUT_OF_RANGE)["minus_subnormal"], dtype=torch.float32) * 24)
    assert float(f) == -1.0


def test_nan_scale_id_raises_in_the_reference():
    """clamp keeps a NaN, NaN + 1 -> long is INT64_MIN, and the table lookup raises (transformer.py:396-400)."""
    table = torch.zeros(4, 8)
    idx = O.scale_index(torch.tensor([float("nan")]), 3)
    assert int(idx[0]) < 0
    with pytest.raises(IndexError):
        table[idx]


def test_bad_rows_names_rows():
    a = torch.arange(12.0).view(4, 3)
    b = a.clone()
    b[2, 1] += 1
    assert ep.bad_rows(a, a) == [] and ep.bad_rows(a, b) == [2]
    b[0, 0] = float("nan")
    assert ep.bad_rows(b, b) == [0] and ep.bad_rows(torch.tensor([[0.0]]), torch.tensor([[-0.0]])) == []
