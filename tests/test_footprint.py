"""The guard-band arena's own arithmetic (tests/footprint.py) on a CPU arena: layout, patterns, violation records, the two-fill protocol."""

import pytest
import torch

from tests import footprint as fp
from tests.footprint import Arena, FootprintError


def _arena(specs):
    a = Arena(fp.arena_bytes(specs), "cpu")
    return a, [a.carve(f"b{i}", *s) for i, s in enumerate(specs)]


def test_layout_alignment_and_guard_sizes():
    specs = [((3, 5, 7), torch.float16), ((1000,), torch.float32), ((515, 1040), torch.bfloat16, 1040 * 2), ((2,), torch.float64)]
    a, views = _arena(specs)
    assert a.mem.numel() == fp.arena_bytes(specs) and a.mem.dtype == torch.uint8
    prev_end = 0
    for i, (v, s) in enumerate(zip(views, specs)):
        b = a.bufs[f"b{i}"]
        assert v.shape == tuple(s[0]) and v.dtype == s[1] and v.data_ptr() % 256 == 0
        assert v.data_ptr() == a.mem.data_ptr() + b.start and b.nbytes == v.numel() * v.element_size()
        pitch = s[0][-1] * v.element_size()
        inner = max(256 * pitch, 64 << 10)
        assert b.start - prev_end >= (inner if i else 4 << 20)                       # in front: its own guard (the outer one for the first)
        if i:
            assert b.start - prev_end >= inner + max(256 * specs[i - 1][0][-1] * views[i - 1].element_size(), 64 << 10)   # + the neighbour's
        prev_end = b.start + b.nbytes
    assert a.nbytes - prev_end >= 4 << 20                                            # the outer guard behind the last buffer
    # the guards tile everything that is not a buffer, without overlap
    covered = torch.zeros(a.nbytes, dtype=torch.int32)
    for r in a.regions:
        covered[r.start:r.start + r.width] += 1
    for b in a.bufs.values():
        covered[b.start:b.start + b.nbytes] += 1
    assert bool((covered == 1).all())
    with pytest.raises(ValueError):
        a.carve("too_much", (1 << 20,), torch.float32)


def test_fill_patterns_are_zero_and_nan():
    a, (h, f, d, i) = _arena([((8,), torch.float16), ((8,), torch.float32), ((8,), torch.float64), ((8,), torch.int32)])
    for v in (h, f, d, i):
        a.fill(v, 0xFF)
    assert bool(torch.isnan(h).all()) and bool(torch.isnan(f).all()) and bool(torch.isnan(d).all()) and bool((i == -1).all())
    bf = h.view(torch.bfloat16)
    assert bool(torch.isnan(bf).all())
    for v in (h, f, d, i):
        a.fill(v, 0x00)
    assert bool((h == 0).all()) and bool((f == 0).all()) and bool((d == 0).all()) and bool((i == 0).all())
    a.fill(f[::2], 0xFF)                                                             # a strided view
    assert bool(torch.isnan(f[::2]).all()) and bool((f[1::2] == 0).all())
    with pytest.raises(AssertionError):
        a.fill(torch.zeros(4), 0x00)                                                 # not a view of the arena


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_violations_name_buffer_side_offset_and_count(byte):
    a, (x, y) = _arena([((4, 16), torch.float32), ((2, 10, 24), torch.float16, 48, 10 * 48)])
    a.fill_guards(byte)
    x.fill_(1.0)
    y.fill_(2.0)
    assert a.violations(byte) == []                                                  # writing the buffers themselves is no violation
    flat = a.mem
    bx, by = a.bufs["b0"], a.bufs["b1"]
    other = 0x5A
    flat[bx.start + bx.nbytes + 64 * 3 + 8] = other                                  # behind x: row 4 + 3, column 2
    flat[bx.start + bx.nbytes + 64 * 3 + 9] = other
    flat[by.start - 5] = other                                                       # in front of y
    flat[a.nbytes - 1] = other                                                       # the last byte of the outer guard
    v = {(r.buffer, r.side): r for r in a.violations(byte)}
    assert set(v) == {("b0", "after"), ("b1", "before"), ("b1", "after")}
    r = v[("b0", "after")]
    assert (r.offset, r.changed, r.where) == (64 * 3 + 8, 2, "row 7 column 2")
    r = v[("b1", "before")]
    assert (r.offset, r.changed) == (-5, 1) and "5 bytes in front" in r.where
    r = v[("b1", "after")]
    assert r.offset == a.nbytes - 1 - (by.start + by.nbytes) and r.changed == 1
    assert "b0 [after] first changed byte at offset 200 (row 7 column 2), 2 bytes changed" in Arena.describe(v.values())
    # a byte equal to the fill is invisible: the reason the protocol uses two patterns
    a.fill_guards(byte)
    flat[by.start - 5] = byte
    assert a.violations(byte) == []


def test_holes_and_scratch():
    M, N, ldo, isz = 6, 8, 12, 2
    a, (out,) = _arena([((2, M + 1, ldo), torch.float16, ldo * isz, (M + 1) * ldo * isz)])
    plane = (M + 1) * ldo * isz
    for pl in range(2):
        a.hole("b0", f"gap columns plane {pl}", pl * plane + N * isz, (ldo - N) * isz, ldo * isz, M)
        a.hole("b0", f"plane gap {pl}", pl * plane + M * ldo * isz, ldo * isz)
    sc = a.scratch("b0", "readable", 0, 4)
    a.fill_guards(0xFF)
    assert bool(torch.isnan(out[:, :M, N:]).all()) and bool(torch.isnan(out[:, M]).all()) and bool(torch.isnan(out[0, 0, :2]).all())
    out[:, :M, :N] = 1.0                                                             # the owned part (and the scratch bytes): fine
    assert a.violations(0xFF) == []
    out[1, 3, N + 1] = 0.5                                                           # a store that ignores the pitch
    out[0, M, 0] = 0.5                                                               # a row behind M
    v = {r.side: r for r in a.violations(0xFF)}
    assert set(v) == {"hole:gap columns plane 1", "hole:plane gap 0"}
    assert v["hole:gap columns plane 1"].where == f"plane 1 row 3 column {N + 1}" and v["hole:gap columns plane 1"].changed == 2
    assert v["hole:gap columns plane 1"].offset == plane + 3 * ldo * isz + (N + 1) * isz
    assert v["hole:plane gap 0"].where == f"plane 0 row {M} column 0"
    a.fill(sc, 0x00)
    assert bool((out[0, 0, :2] == 0).all())
    with pytest.raises(AssertionError):
        a.hole("b0", "outside", 2 * plane - 2, 4)


def test_run_twice_protocol():
    a, (src, dst) = _arena([((64,), torch.float32), ((64,), torch.float32)])
    src.copy_(torch.arange(64.0))
    tail = a.scratch("b0", "value irrelevant", 48 * 4, 16 * 4)

    def good():
        dst[:48] = src[:48] * 2

    a.hole("b1", "not stored", 48 * 4, 16 * 4)
    (got,) = a.run_twice(good, lambda: [dst[:48]])
    assert torch.equal(got, torch.arange(48.0) * 2) and got.data_ptr() != dst.data_ptr()

    def reads_too_far():                                                             # the scratch value reaches an owned output
        dst[:48] = src[:48] * 2
        dst[0] += src[50] * 0

    with pytest.raises(FootprintError) as e:
        a.run_twice(reads_too_far, lambda: [dst[:48]])
    assert list(e.value.mismatch) == [0] and e.value.mismatch[0].nonzero().tolist() == [[0]] and not e.value.violations

    def writes_zero_too_far():                                                       # hides in the 0x00 fill, not in the 0xFF fill
        dst[:49] = 0

    with pytest.raises(FootprintError) as e:
        a.run_twice(writes_zero_too_far, lambda: [dst[:48]])
    (v,) = e.value.violations
    assert (v.buffer, v.side, v.offset, v.changed) == ("b1", "hole:not stored", 48 * 4, 4) and "0xFF" in str(e.value)

    def writes_nan_too_far():                                                        # the other way round
        dst[:48] = 1
        a.mem[a.bufs["b1"].start + 64 * 4] = 0xFF

    with pytest.raises(FootprintError) as e:
        a.run_twice(writes_nan_too_far, lambda: [dst[:48]])
    (v,) = e.value.violations
    assert (v.buffer, v.side, v.offset, v.changed) == ("b1", "after", 0, 1) and "0x00" in str(e.value)

    calls = []
    x = dst[:8]

    def in_place():
        calls.append(float(x[0]))
        x.add_(1.0)

    a.run_twice(in_place, lambda: [x], prepare=lambda: x.fill_(3.0))                 # prepare() restores what a launch consumes
    assert calls == [3.0, 3.0]
    assert tail.kind == "scratch"
