"""The arithmetic of tests/large_offsets.py, without a GPU: every case of tests/test_gpu_large_offsets.py crosses the boundaries it claims, is
the smallest shape that does, fits the memory cap, can fail (a wrapped index lands where the GPU test looks, or leaves the canary at the
true place), and between them the cases and the exclusion table cover every kernel entry the headers declare."""
import glob
import os
import re

import pytest

from tests import large_offsets as L

CASES = list(L.CASES.values())
PAIRS = [pytest.param(c, f, id=f"{c.name}-{f or 'u8'}") for c in CASES for f in c.fmts]
TRANSIENT = 2 << 30          # what a GPU test holds beside the catalogued buffers: one slice of random fp32 input, the fp64 check's operands


def test_the_constants_are_the_boundaries():
    assert L.BOUNDARIES == {L.E30: 2 ** 30, L.E31: 2 ** 31, L.B31: 2 ** 31, L.B32: 2 ** 32}
    assert L.MEM_CAP == 24 * 2 ** 30 and L.SLICE_ROWS == 16384 and L.SLICE_SEQS == 64 and L.EVERY == 4097


@pytest.mark.parametrize("case,fmt", PAIRS)
def test_a_case_crosses_what_it_claims(case, fmt):
    bufs = case.buffers(fmt)
    assert set(case.claims) <= set(bufs)
    for name, b in bufs.items():
        if name in case.claims:
            assert b.crossed() == case.claims[name], (name, b.crossed())
        elif b.role != "work":
            assert b.crossed() == (), (name, "crosses unclaimed", b.crossed())
    tb, tbound = case.target
    assert tbound in case.claims[tb]
    # derived by hand for one buffer of each kind, so that crossed() itself is checked against plain arithmetic
    b = bufs[tb]
    limit = L.BOUNDARIES[tbound]
    reach = b.rows * b.pitch * (b.esize if tbound in (L.B31, L.B32) else 1)
    assert reach > limit


@pytest.mark.parametrize("case,fmt", PAIRS)
def test_a_case_is_the_smallest_that_crosses(case, fmt):
    """One tile, panel, workgroup, sequence, pair or image fewer no longer reaches the target boundary."""
    tb, tbound = case.target
    if case.gran == 0:                           # the ragged image buffers: a fixed layout (large_offsets.ragged_layout)
        esize = case.buffers(fmt)["images"].esize
        off, total = L.ragged_layout(esize)
        nb = [3 * h * w * esize for h, w in L.RAGGED_SIZES]
        assert off[0] == 0 and off[0] + nb[0] < 2 ** 31                                  # image 0: no high bit in any offset
        assert off[1] < 2 ** 32 < off[1] + nb[1] and off[1] % esize == 0                  # image 1 straddles byte 2^32: low word wraps inside it
        assert off[1] >> 32 == 0 and (off[1] + nb[1] - 1) >> 32 == 1
        assert off[2] == off[1] + nb[1] and off[2] >> 32 == 1 and off[2] % esize == 0     # image 2 wholly behind: high word 1 in its table entry
        assert total == off[2] + nb[2] and total - 2 ** 32 < 1 << 22                      # and the buffer ends with it: 2^32 + under 4 MiB
        assert (esize != 1) or (off[1] % 2 == 1)                                          # the u8 gather at an odd byte
        assert L.BOUNDARIES[tbound] < total
        return
    assert tbound in case.buffers(fmt, case.count)[tb].crossed()
    assert tbound not in case.buffers(fmt, case.count - case.gran)[tb].crossed(), (case.count - case.gran, case.unit)


def test_the_shapes_the_issue_names():
    """The counts as plain numbers (the issue's table; the H = 768 LayerNorm is one 4-row workgroup smaller than stated there: 2 796 204 rows
    reach element 2^31, 2 796 200 do not)."""
    n = {c.name: c.count for c in CASES}
    assert n["split"] == 2 ** 31 + 2 ** 20
    assert n["layernorm_768"] == 2_796_204 and n["layernorm_1024"] == 2_097_156
    assert n["gemm_fc1"] == n["gemm_fc2"] == n["rowln"] == 699_136 and n["gemm_tall_x"] == 1_398_272
    assert n["attention"] == n["attention_varlen"] == n["rollout_step"] == n["rollout_step_varlen"] == 1861
    assert n["probs"] == 713 and n["cls_fold"] == n["cls_fold_varlen"] == 5582 and n["images_uniform"] == 11 and n["engine"] == 698
    assert L.CASES["gemm_fc1"].buffers()["out16"].boundary_rows() == [349_524, 349_525, 699_049, 699_050]      # 2^31 bytes in row 349 525; element 2^31 lies in row 699 050: 699 051 rows reach it
    assert L.ATT_ROWS == 932_068
    assert L.CASES["gemm_tall_x"].dims["K"] == {"fp16x3": 64, "bf16": 128}
    e = L.CASES["engine"].buffers()
    assert e["big"].rows == 699_396 and e["big"].rows + e["big"].slack_rows == 699_776


def test_the_ragged_lengths():
    for seed, lengths, nseq, need in ((L.VL_SEED, L.VL_LENGTHS, 1861, 932_068), (L.FOLD_SEED, L.FOLD_LENGTHS, 5582, 2 ** 31 // 768 + 1)):
        assert L.seeded_lengths(nseq, 437, 565, need) == (seed, lengths)
        assert len(lengths) == nseq and min(lengths) >= 437 and max(lengths) <= 565 and len(set(lengths)) > 100
        assert sum(lengths) >= need > sum(lengths[:-1])


@pytest.mark.parametrize("case,fmt", PAIRS)
def test_a_case_fits_the_memory_cap(case, fmt):
    assert case.device_bytes(fmt) + TRANSIENT <= L.MEM_CAP, case.device_bytes(fmt) / 2 ** 30


@pytest.mark.parametrize("case,fmt", PAIRS)
def test_a_case_can_fail(case, fmt):
    """For the first element at or behind each claimed boundary and for the last element of the buffer, in every plane: at least one 32-bit
    form of its index differs from the index, and each that does lands inside the buffer's compared planes -- or, a signed form in the first
    plane only, in front of the buffer, where the true place (canary, or random data of its own) still makes the comparison fail."""
    for name, bounds in case.claims.items():
        b = case.buffers(fmt)[name]
        compared = b.planes * b.plane_stride
        for elem in sorted({b.boundary_elem(x) for x in bounds} | {b.max_elem}):
            for plane in range(b.planes):
                true = plane * b.plane_stride + elem
                landed = b.wraps(elem, plane)
                lost = [k for k, v in landed.items() if v != true]
                assert lost, (name, elem, "no 32-bit form loses a bit: the case crosses nothing")
                for kind in lost:
                    at = landed[kind]
                    if at >= 0:
                        assert at < compared and at < true, (name, kind, at)
                        assert at - plane * b.plane_stride < b.numel or plane > 0, (name, kind, "lands in a gap or in slack rows")
                    else:
                        assert kind.startswith("signed 32-bit") and plane == 0, (name, kind, at)
    # ... and the rows handed to the fp64 check include both sides of every crossing
    rows = set(case.check_rows(fmt))
    for name, bounds in case.claims.items():
        b = case.buffers(fmt)[name]
        if b.rows == max(x.rows for x in case.buffers(fmt).values() if x.role != "work"):
            assert set(b.boundary_rows()) <= rows


def test_check_rows():
    c = L.CASES["gemm_fc1"]
    rows = c.check_rows("fp16x3")
    assert rows[0] == 0 and rows[-1] == 699_135 and 699_049 in rows and 699_050 in rows and 349_525 in rows and 349_524 in rows
    assert set(range(0, 699_136, 4097)) <= set(rows) and len(rows) < 200


def test_every_entry_has_a_case_or_a_reason():
    """Parsed from include/*.h as tests/test_gpu_footprint.py parses its header: an entry added later without a case or a reason fails here."""
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    headers = sorted(glob.glob(os.path.join(inc, "*.h")))
    assert len(headers) >= 7
    declared = set()
    for h in headers:
        declared |= set(re.findall(r"^int\s+(vtq_(?:k|vl)_\w+)\s*\(", open(h).read(), flags=re.M))
    assert {"vtq_k_gemm", "vtq_vl_rollout_step", "vtq_k_gather_patches_u8", "vtq_k_gather_patches_planar", "vtq_k_sample_grid"} <= declared
    covered = {e for c in CASES for e in c.entries if e.startswith("vtq_")}
    assert covered <= declared, covered - declared
    assert not covered & set(L.EXCLUDED) and not (covered | set(L.EXCLUDED)) & L.HOST_ONLY
    assert set(L.EXCLUDED) <= declared and L.HOST_ONLY <= declared
    assert all(len(r) > 20 for r in L.EXCLUDED.values())
    missing = declared - covered - set(L.EXCLUDED) - L.HOST_ONLY
    assert not missing, f"no large-offset case and no reason for: {sorted(missing)}"
