"""Patches placed where a pair differs, on the GPU: vtq_k_diff_cells and vtq_k_sample_weighted (include/vtamiq_hip_weighted_sampler.h),
vtamiq_amd.sampling.sample_patches_weighted and ImagePairVarlenPipeline.submit_images(sampler=WeightedPatchSampler(...)).

The contract every test turns on: the difference pass leaves the WORDS of the restatement's table (tests/weighted_sampler_model.py, which
tests/test_weighted_sampler_model.py holds to the reference's recorded behaviour), the sampler's rows have the BITS of the restatement's for
the same table, a pair's words and a segment's rows depend on nothing else in the batch, and a pipeline that samples this way returns the
bits of submit() fed with the restatement's coordinates."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import sampler_model as SM
from tests import weighted_sampler_model as WM
from tests.footprint import Arena, arena_bytes
from vtamiq_amd import VTAMIQ, _lib, sampling, synth
from vtamiq_amd.patches import extract_patches_varlen
from vtamiq_amd.pipeline import ImagePairVarlenPipeline
from vtamiq_amd.validate import average_over_repeats

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
SEED = 2016
Q = 13107
W = sampling.WeightedPatchSampler


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and bool(torch.isfinite(a).all())


def _model(nscales, cls=VTAMIQ):
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_scales=nscales if nscales > 1 else 0, pretrained=False))
    m = cls(**json.loads(json.dumps(kw)), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 3).items()})
    return m.to(DEV).eval()


def _busy(stream, n=6):
    """Bounded unrelated work on `stream`: n fp32 products of 4096^3."""
    a = torch.ones(4096, 4096, device=DEV)
    torch.mm(a, a)                                                   # the BLAS library's first-use work, on the current stream
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(n):
            torch.mm(a, a)


# ---- the difference pass ---------------------------------------------------------------------------------------------------------------------
def _levels(size, counts, P):
    """[(level, cs, sh, sw)] for counts[l] samples on level l of an image of `size`."""
    return [(l, *WM.geometry(n, size[0] >> l, size[1] >> l, P)) for l, n in enumerate(counts) if n]


def _pack(pairs, lead=1, gap=0):
    """The pairs' images back to back in one byte buffer -- the references, then the distorted images -- behind `lead` bytes and `gap` bytes
    apart: (bytes, [a offsets], [b offsets])."""
    parts, offs, at = [np.full(lead, 0x5A, np.uint8)], [], lead
    for im in [a for a, _ in pairs] + [b for _, b in pairs]:
        offs.append(at)
        parts += [im.reshape(-1), np.full(gap, 0xA5, np.uint8)]
        at += im.size + gap
    return np.concatenate(parts), offs[:len(pairs)], offs[len(pairs):]


def _tables(pairs, levels, offs_a, offs_b, P):
    """(want: the restatement's table, pairs int64 [NP, 8], lev int32 [NL, 8])."""
    want, lev, heads = WM.diff_table(pairs, levels, P)
    pt = np.zeros((len(pairs), 8), np.int64)
    row = 0
    for p, ((a, _), rows) in enumerate(zip(pairs, levels)):
        pt[p] = (offs_a[p], offs_b[p], a.shape[0], a.shape[1], heads[p], row, len(rows), 0)
        row += len(rows)
    return want, pt, lev


def _diff(pairs, levels, P=16, lead=1, gap=0):
    flat, oa, ob = _pack(pairs, lead, gap)
    want, pt, lev = _tables(pairs, levels, oa, ob, P)
    tab = torch.full((len(want),), -1, dtype=I64, device=DEV)
    sampling.launch_diff_cells(torch.from_numpy(flat).to(DEV), torch.from_numpy(pt).to(DEV), torch.from_numpy(lev).to(DEV), pt, lev, P, tab, len(want))
    torch.cuda.synchronize()
    return tab.cpu().numpy().view(np.uint64), want


def _diff_cases():
    rs = np.random.RandomState(41)
    pair = lambda h, w, **kw: WM.image_pair(rs, h, w, **kw)
    cases = [("17 x 40: one row of cells, extent 1", pair(17, 40), [5], 16),
             ("33 x 47: odd", pair(33, 47), [6], 16),
             ("64 x 64", pair(64, 64), [10], 16),
             ("96 x 128, three levels", pair(96, 128), [20, 8, 4], 16),
             ("97 x 131, three levels, a row and columns dropped at every pooled level", pair(97, 131), [20, 8, 4], 16),
             ("16 x 64: extent 0", pair(16, 64), [4], 16),
             ("Ra != Rb", pair(48, 56, lo_a=10, hi_a=250, lo_b=30, hi_b=235), [12], 16),
             ("40 x 300: two tiles across, P = 8, two levels", pair(40, 300), [40, 10], 8)]
    a, b = pair(40, 56)
    cases.append(("a constant image: Ra = 0", (np.full_like(a, 77), b), [8], 16))
    cases.append(("a constant distorted image: Rb = 0", (a, np.full_like(b, 200)), [8], 16))
    cases.append(("identical images: variance 0", (a, a.copy()), [8], 16))
    a = rs.randint(0, 256, size=(64, 64, 3)).astype(np.uint8)
    a[0, 0], a[1, 1] = 0, 255
    b = a.copy()
    b[25, 25] = (a[25, 25].astype(np.int64) + 128) % 256              # rows and columns 24 .. 26 lie in the windows of cells 0, 1 and 2 (cs = 12)
    cases.append(("one differing pixel that 3 x 3 windows share", (a, b), [30], 16))
    return cases


DIFF_CASES = _diff_cases()


@pytest.mark.parametrize("case", DIFF_CASES, ids=[c[0] for c in DIFF_CASES])
def test_difference_pass_has_the_words_of_the_restatement(case):
    name, pair, counts, P = case
    levels = _levels(pair[0].shape, counts, P)
    for lead in (1, 4):                                              # the first image at an odd and at an aligned address
        got, want = _diff([pair], [levels], P, lead=lead)
        assert np.array_equal(got, want), (name, lead, np.flatnonzero(got != want)[:8])
    if "3 x 3" in name:
        cs, sh, sw = levels[0][1:]
        cells = want[6:].reshape(sh, sw)
        assert cs == 12 and int(want[4]) > 0 and (cells[:3, :3] == want[4]).all() and cells.sum() == 9 * want[4]
    if "extent 0" in name:
        assert levels[0][2] == 1 and levels[0][1] * 0 == pair[0].shape[0] - P
    if "extent 1" in name:
        assert levels[0][2] == 1 and pair[0].shape[0] - P == 1
    if "= 0" in name or "identical" in name:
        assert not want[4:].any()


def test_twelve_pairs_in_one_launch_are_the_pairs_alone():
    """All twelve catalogue pairs of one patch size... the eleven of P = 16 and one more, packed back to back at odd byte offsets, in one
    launch: every pair's words are those of the pair alone (which the test above compares with the restatement)."""
    picked = [c for c in DIFF_CASES if c[3] == 16]
    rs = np.random.RandomState(43)
    picked.append(("one more", WM.image_pair(rs, 35, 51), [7], 16))
    assert len(picked) == 12
    pairs, levels = [c[1] for c in picked], [_levels(c[1][0].shape, c[2], 16) for c in picked]
    flat, oa, ob = _pack(pairs)
    assert sum(o % 2 for o in oa + ob) >= 8
    got, want = _diff(pairs, levels)
    assert np.array_equal(got, want)
    at = 0
    for pr, lv in zip(pairs, levels):
        alone, _ = _diff([pr], [lv])
        assert np.array_equal(alone, got[at:at + len(alone)])
        at += len(alone)
    assert at == len(got)


# ---- the sampler on synthetic tables --------------------------------------------------------------------------------------------------------
def _seg_rows(specs):
    """specs: [(n, cs, sh, sw, hm, wm, level, head, off)] -> int32 [NS, 12] with the first rows filled in."""
    rows, first = [], 0
    for n, cs, sh, sw, hm, wm, level, head, off in specs:
        rows.append((first, n, cs, sh, sw, hm, wm, level, head, off, 0, 0))
        first += n
    return np.asarray(rows, np.int32).reshape(-1, 12), first


def _sample(specs, keys, tab, dw, uw, P=16, seed=SEED, q=Q, ids=True):
    seg, total = _seg_rows(specs)
    keys = np.asarray([int(k) % (1 << 64) for k in keys], np.uint64)
    smp = torch.full((total, 2), -1, dtype=I32, device=DEV)
    sid = torch.full((total,), -1, dtype=I32, device=DEV) if ids else None
    dtab = torch.from_numpy(np.asarray(tab, np.uint64).view(np.int64)).to(DEV) if tab is not None else None
    dseg, dkeys = torch.from_numpy(seg).to(DEV), torch.from_numpy(keys.view(np.int64)).to(DEV)
    rc = _lib.load().vtq_k_sample_weighted(dseg.data_ptr(), dkeys.data_ptr(),
                                           seg.ctypes.data_as(C.POINTER(C.c_int32)), keys.ctypes.data_as(C.POINTER(C.c_uint64)), len(seg), P,
                                           dtab.data_ptr() if dtab is not None else None, len(tab) if tab is not None else 0, dw, uw, seed, q,
                                           smp.data_ptr(), sid.data_ptr() if ids else None, _stream())
    assert rc == 0, _lib.load().vtq_last_error().decode()
    torch.cuda.synchronize()
    return smp.cpu().numpy(), (sid.cpu().numpy() if ids else None)


def _want(specs, keys, tab, dw, uw, P=16, seed=SEED, q=Q):
    segs = [WM.segment(seed, k, level, n, cs, sh, sw, hm, wm, P, q, dw, uw, tab, head, off) for (n, cs, sh, sw, hm, wm, level, head, off), k in zip(specs, keys)]
    return np.concatenate([s.samples for s in segs]), np.concatenate([np.full(len(s.samples), sp[6], np.int32) for s, sp in zip(segs, specs)]), segs


def _spec(h, w, n, P=16, level=0, head=-1, off=-1):
    cs, sh, sw = WM.geometry(n, h, w, P)
    return (n, cs, sh, sw, h - P, w - P, level, head, off)


def _synthetic():
    """name -> (specs, table, dw, uw, P, check(segments))."""
    out = {}
    hot = lambda h, w, n, P=16: WM.map_table(WM.hot_spot_map(h, w), *WM.geometry(n, h, w, P), P)
    E = lambda s: int(s.k_ceil.sum()) - len(s.samples)
    out["E = 0: two equal cells"] = ([_spec(16, 40, 4)], None, 0.0, 1.0, 16, lambda s: E(s[0]) == 0 and s[0].k.tolist() == [2, 2])
    out["n = 1: E = cells - 1"] = ([_spec(64, 64, 1, head=0, off=4)], hot(64, 64, 1), 1.0, 1.0, 16, lambda s: E(s[0]) == np.count_nonzero(s[0].k_ceil) - 1 == 15)
    out["one cell"] = ([_spec(17, 21, 4, head=0, off=4)], hot(17, 21, 4), 1.0, 0.1, 16, lambda s: s[0].k.tolist() == [4])
    m = np.zeros((64, 64), np.int64)
    m[:5, :5] = 100
    out["all weight in one cell, uw = 0: k = n = 300"] = ([_spec(64, 64, 300, head=0, off=4)], WM.map_table(m, *WM.geometry(300, 64, 64, 16), 16), 1.0, 0.0, 16,
                                                           lambda s: s[0].use and s[0].k[0] == 300 and s[0].k.sum() == 300)
    out["all weight in one cell, uw = 0: k = n = 8100, the limit (wd = 90)"] = ([_spec(64, 64, 8100, head=0, off=4)], WM.map_table(m, *WM.geometry(8100, 64, 64, 16), 16), 1.0, 0.0,
                                                                                 16, lambda s: s[0].use and s[0].k[0] == 8100)
    out["cs at its lower clip, last extents cs"] = ([_spec(64, 64, 300, head=0, off=4)], hot(64, 64, 300), 1.0, 0.1, 16,
                                                    lambda s: WM.geometry(300, 64, 64, 16) == (12, 4, 4))
    out["cs at its upper clip"] = ([_spec(96, 128, 4, head=0, off=4)], hot(96, 128, 4), 1.0, 0.1, 16, lambda s: WM.geometry(4, 96, 128, 16)[0] == 24)
    out["last extents 1 (rows) and 12 = cs (columns)"] = ([_spec(17, 40, 9, head=0, off=4)], hot(17, 40, 9), 1.0, 0.5, 16,
                                                          lambda s: WM.extents(1, 12, 1)[-1] == 1 and WM.extents(24, 12, 2)[-1] == 12)
    out["extent 0"] = ([_spec(16, 64, 7, head=0, off=4)], hot(16, 64, 7), 1.0, 0.5, 16, lambda s: (s[0].samples[:, 0] == 0).all())
    out["P = 8, odd"] = ([_spec(45, 77, 60, 8, head=0, off=4)], hot(45, 77, 60, 8), 1.0, 0.2, 8, lambda s: s[0].use)
    out["713 cells: the sixteen-wave launch"] = ([_spec(384, 512, 3000, head=0, off=4)], hot(384, 512, 3000), 1.0, 0.1, 16,
                                                 lambda s: len(s[0].k) == 713 and s[0].use)
    out["NULL table, dw = 0: the uniform perturbed grid"] = ([_spec(96, 128, 50), _spec(48, 64, 12, level=1)], None, 0.0, 1.0, 16, lambda s: not s[0].use)
    return out


SYNTHETIC = _synthetic()


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_sampler_has_the_bits_of_the_restatement(name):
    specs, tab, dw, uw, P, check = SYNTHETIC[name]
    for key in (0, 2 ** 63 + 5):
        keys = [key + i for i in range(len(specs))]
        got = _sample(specs, keys, tab, dw, uw, P)
        want = _want(specs, keys, tab, dw, uw, P)
        assert check(want[2]), (name, "the case is not the edge it names")
        assert np.array_equal(got[0], want[0]), (name, key, np.flatnonzero((got[0] != want[0]).any(axis=1))[:8])
        assert np.array_equal(got[1], want[1])


def test_three_levels_on_the_table_of_the_difference_pass():
    """sample_patches_weighted end to end: the difference pass's table feeds the sampler, three levels, two pairs, aligned and not; the
    lists go straight into extract_patches_varlen(validate=False)."""
    rs = np.random.RandomState(47)
    pairs = [WM.image_pair(rs, 128, 160), WM.image_pair(rs, 125, 159, lo_a=5, hi_a=240)]
    refs, dists = [a for a, _ in pairs], [b for _, b in pairs]
    flat, oa, ob = _pack(pairs, lead=0)
    dflat = torch.from_numpy(flat).to(DEV)
    sizes = [a.shape[:2] for a in refs]
    for aligned, keys in ((True, [3, 4]), (False, [3, 4, 5, 2 ** 64 - 1])):
        smp, sid, lengths = sampling.sample_patches_weighted(dflat, oa + ob, sizes, [30, 41], keys, W(1.0, 0.1), SEED, 3, aligned=aligned)
        torch.cuda.synchronize()
        want_smp, want_sid = WM.pair_batch(refs, dists, [30, 41], keys, SEED, 1.0, 0.1, 3, aligned=aligned)
        assert lengths == [30, 41, 30, 41] and set(np.concatenate(want_sid).tolist()) == {0, 1, 2}
        assert np.array_equal(smp.cpu().numpy(), np.concatenate(want_smp)) and np.array_equal(sid.cpu().numpy(), np.concatenate(want_sid))
        assert np.array_equal(want_smp[0], want_smp[2]) == aligned
        got = extract_patches_varlen(dflat, smp, lengths, sid, 3, validate=False, sizes=sizes * 2)
        ref = extract_patches_varlen(dflat, torch.from_numpy(np.concatenate(want_smp)), lengths, torch.from_numpy(np.concatenate(want_sid)), 3,
                                     validate=True, sizes=sizes * 2)
        assert all(same(g, r) for g, r in zip(got, ref))
    # diff_weight = 0, the class's default: the uniform perturbed grid on the same plan, no table and no pixel read
    for sampler in (W(), W(0.0, 0.3)):
        smp, sid, lengths = sampling.sample_patches_weighted(dflat, oa + ob, sizes, [30, 41], [3, 4], sampler, SEED, 3)
        torch.cuda.synchronize()
        uni_smp, uni_sid = WM.pair_batch(refs, dists, [30, 41], [3, 4], SEED, 0.0, 1.0, 3)
        assert np.array_equal(smp.cpu().numpy(), np.concatenate(uni_smp)) and np.array_equal(sid.cpu().numpy(), np.concatenate(uni_sid))
        assert not np.array_equal(np.concatenate(uni_smp), np.concatenate(WM.pair_batch(refs, dists, [30, 41], [3, 4], SEED, 1.0, 0.1, 3)[0]))
    # the region that differs (rows 42 .. 73, columns 80 .. 119 of the first pair: 1 / 16 of the image) gets level 0's patches
    s0 = want_smp[0][want_sid[0] == 0].astype(np.int64)
    touching = ((s0[:, 0] + 16 > 42) & (s0[:, 0] < 74) & (s0[:, 1] + 16 > 80) & (s0[:, 1] < 120)).mean()
    assert touching > 0.5, touching


def test_a_segment_does_not_depend_on_its_batch_or_the_workgroup_size():
    """Eight segments alone, in a batch of 40 (five times, other keys around them) and beside a segment of 713 cells, which launches every
    workgroup of the batch with sixteen waves instead of four."""
    names = ["n = 1: E = cells - 1", "one cell", "cs at its lower clip, last extents cs", "cs at its upper clip",
             "last extents 1 (rows) and 12 = cs (columns)", "extent 0", "all weight in one cell, uw = 0: k = n = 300", "E = 0: two equal cells"]
    tabs, specs, at = [], [], 0
    for nm in names:
        sp, tab, *_ = SYNTHETIC[nm]
        tab = tab if tab is not None else np.zeros(0, np.uint64)
        n, cs, sh, sw, hm, wm, level, head, off = sp[0]
        specs.append((n, cs, sh, sw, hm, wm, level, head + at if head >= 0 else -1, off + at if off >= 0 else -1))
        tabs.append(tab)
        at += len(tab)
    tab = np.concatenate(tabs)
    keys = [100 + i for i in range(8)]
    alone = [_sample([sp], [k], tab, 1.0, 0.3)[0] for sp, k in zip(specs, keys)]
    want = _want(specs, keys, tab, 1.0, 0.3)
    assert np.array_equal(np.concatenate(alone), want[0])
    batch, _ = _sample(specs * 5, [k + 1000 * r for r in range(5) for k in keys], tab, 1.0, 0.3)
    assert len(specs * 5) == 40 and np.array_equal(batch[:len(want[0])], want[0]) and not np.array_equal(batch[len(want[0]):2 * len(want[0])], want[0])
    big_spec, big_tab, *_ = SYNTHETIC["713 cells: the sixteen-wave launch"]
    n, cs, sh, sw, hm, wm, level, head, off = big_spec[0]
    both, _ = _sample(specs + [(n, cs, sh, sw, hm, wm, level, head + at, off + at)], keys + [9], np.concatenate([tab, big_tab]), 1.0, 0.3)
    assert np.array_equal(both[:len(want[0])], want[0])


# ---- footprint and refusals -----------------------------------------------------------------------------------------------------------------
class DiffEntry:
    """vtq_k_diff_cells on a guard-band arena: the images with holes between them, the tables and the weight table at the header's extents."""

    def __init__(self, pairs, counts, P=16, gap=37):
        self.P = P
        levels = [_levels(a.shape, c, P) for (a, _), c in zip(pairs, counts)]
        flat, oa, ob = _pack(pairs, lead=0, gap=gap)
        flat = flat[:len(flat) - gap]                               # the buffer ends with the last image's last byte
        self.want, self.pt, self.lev = _tables(pairs, levels, oa, ob, P)
        specs = [("images", (len(flat),), U8), ("pairs", (len(pairs), 8), I64), ("lev", (len(self.lev), 8), I32), ("tab", (len(self.want),), I64)]
        self.arena = Arena(arena_bytes([s[1:] for s in specs]), DEV)
        self.b = {name: self.arena.carve(name, shape, dtype) for name, shape, dtype in specs}
        self.b["images"].copy_(torch.from_numpy(flat))
        self.b["pairs"].copy_(torch.from_numpy(self.pt))
        self.b["lev"].copy_(torch.from_numpy(self.lev))
        for k, (im, o) in enumerate(zip([a for a, _ in pairs] + [b for _, b in pairs], oa + ob)):
            if o + im.size < len(flat):
                self.arena.hole("images", f"gap {k}", o + im.size, gap)
        torch.cuda.synchronize()

    def call(self, **kw):
        b = self.b
        a = dict(images=b["images"].data_ptr(), nbytes=b["images"].numel(), pairs=b["pairs"].data_ptr(), lev=b["lev"].data_ptr(), pairs_host=self.pt,
                 lev_host=self.lev, NP=len(self.pt), NL=len(self.lev), P=self.P, tab=b["tab"].data_ptr(), words=len(self.want))
        a.update(kw)
        ph = a["pairs_host"].ctypes.data_as(C.POINTER(C.c_int64)) if a["pairs_host"] is not None else None
        lh = a["lev_host"].ctypes.data_as(C.POINTER(C.c_int32)) if a["lev_host"] is not None else None
        lib = _lib.load()
        rc = lib.vtq_k_diff_cells(a["images"], a["nbytes"], a["pairs"], a["lev"], ph, lh, a["NP"], a["NL"], a["P"], a["tab"], a["words"], _stream())
        return rc, lib.vtq_last_error().decode()


def _footprint_pairs():
    rs = np.random.RandomState(53)
    return [WM.image_pair(rs, 33, 47), WM.image_pair(rs, 96, 128), WM.image_pair(rs, 17, 40), WM.image_pair(rs, 40, 300)], [[6], [20, 8, 4], [5], [40]]


def test_difference_pass_footprint():
    """Guards and the 37-byte gaps between the images filled with 0x00, then 0xFF: exactly the table's words are written, no guard byte
    changes, the table is bit-identical across the fills -- no byte outside an image reaches a result, though every image starts and ends
    inside a dword that holds a neighbour's bytes -- and equals the restatement."""
    e = DiffEntry(*_footprint_pairs())

    def launch():
        e.arena.fill(e.b["tab"], 0xFF)
        rc, msg = e.call()
        assert rc == 0, msg

    got = e.arena.run_twice(launch, lambda: [e.b["tab"]])
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), e.want)


def test_refused_difference_passes_leave_every_buffer_untouched():
    e = DiffEntry(*_footprint_pairs())
    e.arena.fill(e.b["tab"], 0xFF)
    e.arena.fill_guards(0x00)
    torch.cuda.synchronize()
    before = e.arena.mem.clone()

    def lev(row, col, value):
        t = e.lev.copy()
        t[row, col] = value
        return dict(lev_host=t)

    def pair(row, col, value):
        t = e.pt.copy()
        t[row, col] = value
        return dict(pairs_host=t)

    cases = {k: {k: None} for k in ("images", "pairs", "lev", "pairs_host", "lev_host", "tab")}
    cases.update({"NP < 1": dict(NP=0), "NL short": dict(NL=len(e.lev) - 1), "P = 4": dict(P=4), "lev unaligned": dict(lev=e.b["lev"].data_ptr() + 4),
                  "image leaves the buffer": pair(3, 1, int(e.pt[3, 1]) + 1), "negative offset": pair(0, 0, -1), "2^22 pixels": pair(1, 2, 1 << 21),
                  "image below a patch": pair(2, 2, 15), "head": pair(1, 4, 5), "first lev row": pair(1, 5, 2), "lev rows": pair(1, 6, 2),
                  "pair order": lev(1, 0, 2), "level 4": lev(3, 1, 4), "level repeats": lev(2, 1, 0), "level below a patch": lev(0, 1, 2),
                  "cs below 3 P / 4": lev(0, 2, 11), "sh": lev(0, 3, 3), "sw": lev(1, 4, 1), "tab_off": lev(2, 6, 1), "lev head": lev(2, 5, 4),
                  "tab_words": dict(words=len(e.want) + 1)})
    for name, kw in cases.items():
        rc, msg = e.call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_diff_cells:"), (name, rc, msg)
    torch.cuda.synchronize()
    assert e.arena.violations(0x00) == []
    assert torch.equal(e.arena.mem, before), "a refused call wrote to the device"
    rc, msg = e.call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(e.b["tab"].cpu().numpy().view(np.uint64), e.want)


class SampleEntry:
    """vtq_k_sample_weighted on a guard-band arena."""

    def __init__(self, specs, keys, tab):
        self.seg, total = _seg_rows(specs)
        self.keys = np.asarray(keys, np.uint64)
        self.tab = np.asarray(tab, np.uint64)
        sp = [("seg", (len(self.seg), 12), I32), ("keys", (len(keys),), I64), ("tab", (len(tab),), I64), ("samples", (total, 2), I32), ("scale_ids", (total,), I32)]
        self.arena = Arena(arena_bytes([s[1:] for s in sp]), DEV)
        self.b = {name: self.arena.carve(name, shape, dtype) for name, shape, dtype in sp}
        self.b["seg"].copy_(torch.from_numpy(self.seg))
        self.b["keys"].copy_(torch.from_numpy(self.keys.view(np.int64)))
        self.b["tab"].copy_(torch.from_numpy(self.tab.view(np.int64)))
        torch.cuda.synchronize()

    def outputs(self):
        return [self.b["samples"], self.b["scale_ids"]]

    def call(self, **kw):
        b = self.b
        a = dict(seg=b["seg"].data_ptr(), keys=b["keys"].data_ptr(), seg_host=self.seg, keys_host=self.keys, NS=len(self.seg), P=16, tab=b["tab"].data_ptr(),
                 words=len(self.tab), dw=1.0, uw=0.1, seed=SEED, q=Q, samples=b["samples"].data_ptr(), scale_ids=b["scale_ids"].data_ptr())
        a.update(kw)
        sh = a["seg_host"].ctypes.data_as(C.POINTER(C.c_int32)) if a["seg_host"] is not None else None
        kh = a["keys_host"].ctypes.data_as(C.POINTER(C.c_uint64)) if a["keys_host"] is not None else None
        lib = _lib.load()
        rc = lib.vtq_k_sample_weighted(a["seg"], a["keys"], sh, kh, a["NS"], a["P"], a["tab"], a["words"], a["dw"], a["uw"], a["seed"], a["q"],
                                       a["samples"], a["scale_ids"], _stream())
        return rc, lib.vtq_last_error().decode()


def _sample_entry():
    rs = np.random.RandomState(59)
    pair = WM.image_pair(rs, 96, 128)
    levels = _levels((96, 128), [20, 8, 4], 16)
    tab, lev, heads = WM.diff_table([pair], [levels], 16)
    specs = [(n, cs, sh, sw, (96 >> l) - 16, (128 >> l) - 16, l, 0, int(off)) for (l, cs, sh, sw), n, off in zip(levels, [20, 8, 4], lev[:, 6])]
    specs = specs + [_spec(64, 64, 40)] + specs                      # the pair's two images around an image without a table
    return SampleEntry(specs, [7, 7, 7, 8, 9, 9, 9], tab), specs


def test_sampler_footprint():
    e, specs = _sample_entry()

    def launch():
        for out in e.outputs():
            e.arena.fill(out, 0xFF)
        rc, msg = e.call()
        assert rc == 0, msg

    got = e.arena.run_twice(launch, e.outputs)
    want = _want(specs, e.keys.tolist(), e.tab, 1.0, 0.1)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    assert not np.array_equal(want[0][:32], want[0][72:]) and want[2][0].use and not want[2][3].use


def test_refused_samplings_leave_every_buffer_untouched():
    e, specs = _sample_entry()
    for out in e.outputs():
        e.arena.fill(out, 0xFF)
    e.arena.fill_guards(0x00)
    torch.cuda.synchronize()
    before = e.arena.mem.clone()

    def edit(row, col, value):
        t = e.seg.copy()
        t[row, col] = value
        return dict(seg_host=t)

    cases = {k: {k: None} for k in ("seg", "keys", "seg_host", "keys_host", "samples")}
    cases.update({"NS < 1": dict(NS=0), "P = 4": dict(P=4), "n < 1": edit(1, 1, 0), "n > 8100": edit(0, 1, 8101), "cs": edit(0, 2, 11), "sh": edit(0, 3, 9),
                  "sw": edit(0, 4, 1), "cells": edit(0, 3, 9000), "negative h - P": edit(0, 5, -1), "level 4": edit(0, 7, 4), "first row": edit(2, 0, 0),
                  "scale_ids NULL with levels": dict(scale_ids=None), "amount_q": dict(q=1 << 16), "seg unaligned": dict(seg=e.b["seg"].data_ptr() + 4),
                  "negative weight": dict(dw=-1.0), "nan weight": dict(uw=float("nan")), "no weight": dict(dw=0.0, uw=0.0), "head beyond the table": edit(0, 8, len(e.tab) - 3),
                  "tab_off beyond the table": edit(2, 9, len(e.tab) - 2), "half a table": edit(0, 8, -1), "tab NULL with dw > 0": dict(tab=None)})
    for name, kw in cases.items():
        rc, msg = e.call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_sample_weighted:"), (name, rc, msg)
    torch.cuda.synchronize()
    assert e.arena.violations(0x00) == []
    assert torch.equal(e.arena.mem, before), "a refused call wrote to the device"
    rc, msg = e.call(tab=None, dw=0.0, uw=1.0)                       # allowed: no pixel is needed
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(e.b["samples"].cpu().numpy(), _want(specs, e.keys.tolist(), None, 0.0, 1.0)[0])


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------
PIPE_SIZES = [(48, 64), (96, 128), (80, 80)]                         # one, two and two levels when three are asked for


def _pairs(rs, mix):
    prs = [WM.image_pair(rs, *PIPE_SIZES[k]) for k in mix]
    return [a for a, _ in prs], [b for _, b in prs]


def _cap(pairs, count, nscales, repeats=1):
    return dict(max_pairs=pairs * repeats, max_image_bytes=2 * 3 * 96 * 128 * pairs, max_patches=pairs * count * repeats, num_scales=nscales)


@pytest.mark.parametrize("nscales,side_stream", [(1, False), (3, False), (3, True)], ids=["1-scale", "3-scales", "3-scales-side-stream"])
def test_submit_images_weighted_has_the_bits_of_submit_with_the_restatements_coordinates(nscales, side_stream):
    """Three batches over two slots: six pairs of three sizes, aligned; the same unaligned (two keys on the pair's one table); three pairs
    again on the first slot.  Each equals submit() fed with the restatement's coordinates; pairs of two sizes and the group entry are
    refused by name with nothing enqueued."""
    m = _model(nscales)
    rs = np.random.RandomState(61)
    count, sampler = 40, W(1.0, 0.1)
    batches = [(_pairs(rs, [0, 1, 2, 2, 1, 0]), True, list(range(10, 16))), (_pairs(rs, [0, 1, 2, 2, 1, 0]), False, list(range(20, 32))),
               (_pairs(rs, [2, 0, 1]), True, [2 ** 63, 1, 2])]

    def run():
        pipe = ImagePairVarlenPipeline(m, **_cap(6, count, nscales))
        got, want = [], []
        for (refs, dists), aligned, keys in batches:
            got.append(pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, aligned=aligned, sampler=sampler))
            smp, sid = WM.pair_batch(refs, dists, count, keys, SEED, 1.0, 0.1, nscales, aligned=aligned)
            want.append(pipe.submit(refs, dists, smp, scale_ids=sid if nscales > 1 else None))
        slot = pipe.count
        (refs, dists), _, keys = batches[2]
        with pytest.raises(ValueError, match="one size"):
            pipe.submit_images(refs, dists[1:] + dists[:1], count, keys=keys * 2, seed=SEED, aligned=False, sampler=sampler)
        with pytest.raises(NotImplementedError, match="WeightedPatchSampler"):
            pipe.submit_group_images(refs, dists, [0, 1, 2], count, sampler=sampler)
        assert pipe.count == slot, "a refused batch took a slot"
        return got, want

    if side_stream:
        side = torch.cuda.Stream()
        _busy(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            got, want = run()
    else:
        got, want = run()
    torch.cuda.synchronize()
    for it, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (len(batches[it][0][0]),) and same(g, w), it
    assert not torch.equal(got[0], got[1])


def test_num_repeats_weighted_has_the_bits_of_the_explicit_batch_averaged():
    m = _model(3)
    rs = np.random.RandomState(67)
    refs, dists = _pairs(rs, [1, 2, 0])
    keys, count, R = [3, 2 ** 64 - 1, 5], 36, 3
    pipe = ImagePairVarlenPipeline(m, **_cap(3, count, 3, repeats=R))
    q = pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, num_repeats=R, sampler=W(1.0, 0.1))
    keys3 = [sampling.repeat_key(k, r) for r in range(R) for k in keys]
    smp, sid = WM.pair_batch(refs * R, dists * R, count, keys3, SEED, 1.0, 0.1, 3)
    explicit = ImagePairVarlenPipeline(m, max_pairs=3 * R, max_image_bytes=R * 2 * 3 * 96 * 128 * 3, max_patches=3 * R * count, num_scales=3)
    q3 = explicit.submit(refs * R, dists * R, smp, scale_ids=sid)
    torch.cuda.synchronize()
    assert q3.shape == (9,) and not torch.equal(q3[:3], q3[3:6])
    assert q.dtype == torch.float64 and q.shape == (3,) and same(q, average_over_repeats(q3, R))


@pytest.mark.parametrize("nscales", [1, 3])
def test_submit_images_without_a_difference_weight_is_the_uniform_perturbed_grid(nscales):
    """WeightedPatchSampler() -- diff_weight 0, the class's default -- through the pipeline, aligned, unaligned and with repeats: the bits
    of submit() with the restatement's uniform coordinates; no table is read (the segments carry none)."""
    m = _model(nscales)
    rs = np.random.RandomState(73)
    refs, dists = _pairs(rs, [1, 0, 2])
    count, R = 33, 2
    pipe = ImagePairVarlenPipeline(m, **_cap(3, count, nscales, repeats=R))
    for aligned, keys in ((True, [1, 2, 3]), (False, [1, 2, 3, 4, 5, 6])):
        got = pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, aligned=aligned, sampler=W())
        smp, sid = WM.pair_batch(refs, dists, count, keys, SEED, 0.0, 1.0, nscales, aligned=aligned)
        want = pipe.submit(refs, dists, smp, scale_ids=sid if nscales > 1 else None)
        torch.cuda.synchronize()
        assert same(got, want), aligned
    q = pipe.submit_images(refs, dists, count, keys=[1, 2, 3], seed=SEED, num_repeats=R, sampler=W(0.0, 2.0))
    keys2 = [sampling.repeat_key(k, r) for r in range(R) for k in [1, 2, 3]]
    smp, sid = WM.pair_batch(refs * R, dists * R, count, keys2, SEED, 0.0, 1.0, nscales)
    explicit = ImagePairVarlenPipeline(m, max_pairs=3 * R, max_image_bytes=R * 2 * 3 * 96 * 128 * 3, max_patches=3 * R * count, num_scales=nscales)
    q2 = explicit.submit(refs * R, dists * R, smp, scale_ids=sid if nscales > 1 else None)
    torch.cuda.synchronize()
    assert same(q, average_over_repeats(q2, R))


def test_the_default_sampler_keeps_its_bits_beside_the_weighted_one():
    """submit_images() without a sampler, before and after a weighted submission on the same pipeline: the bits of submit() with the
    default sampler's restatement (tests/sampler_model.py), which tests/test_gpu_sampler.py pinned before the weighted sampler existed.
    With VTQ_PARENT_LIB=<a build of the parent commit's library> the comparison is also made against that library itself (it lacks the
    new entries, so vtamiq_amd._lib binds it only with VTQ_ALLOW_ABI_MISMATCH=1 beside it)."""
    m = _model(3)
    rs = np.random.RandomState(71)
    refs, dists = _pairs(rs, [0, 1, 2])
    keys, count = [5, 6, 7], 30
    pipe = ImagePairVarlenPipeline(m, **_cap(3, count, 3))
    first = pipe.submit_images(refs, dists, count, keys=keys, seed=SEED)
    pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, sampler=W(1.0, 0.1))
    again = pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, sampler=sampling.PatchSampler())
    smp, sid = SM.per_image([r.shape[:2] for r in refs], count, keys, SEED, 3)
    want = pipe.submit(refs, dists, smp, scale_ids=sid)
    torch.cuda.synchronize()
    assert same(first, want) and same(again, want)
    # given another build of the library in VTQ_PARENT_LIB (the parent commit's): its sampler's rows and its engine's scores, bit for bit
    parent = os.environ.get("VTQ_PARENT_LIB")
    if parent:
        class ParentVTAMIQ(VTAMIQ):
            def _engine_lib(self):
                return _lib.load(parent)

        sizes = [r.shape[:2] for r in refs]
        plan = sampling.plan_samples(sizes, count, 3)
        seg, seg_keys = np.ascontiguousarray(plan.seg), np.ascontiguousarray(np.asarray(keys, np.uint64)[plan.seg_image])
        dseg, dkeys = torch.from_numpy(seg).to(DEV), torch.from_numpy(seg_keys.view(np.int64)).to(DEV)
        rows = {}
        for name, lib in (("parent", _lib.load(parent)), ("this", _lib.load())):
            o_smp, o_sid = torch.full((plan.total, 2), -1, dtype=I32, device=DEV), torch.full((plan.total,), -1, dtype=I32, device=DEV)
            rc = lib.vtq_k_sample_grid(dseg.data_ptr(), dkeys.data_ptr(), seg.ctypes.data_as(C.POINTER(C.c_int32)),
                                       seg_keys.ctypes.data_as(C.POINTER(C.c_uint64)), len(seg), SEED, Q, o_smp.data_ptr(), o_sid.data_ptr(), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            rows[name] = (o_smp.cpu().numpy(), o_sid.cpu().numpy())
        assert np.array_equal(rows["parent"][0], rows["this"][0]) and np.array_equal(rows["parent"][1], rows["this"][1])
        assert np.array_equal(rows["parent"][0], np.concatenate(smp))
        cut = np.cumsum([count] * len(refs))[:-1]
        old_pipe = ImagePairVarlenPipeline(_model(3, ParentVTAMIQ), **_cap(3, count, 3))
        old_q = old_pipe.submit(refs, dists, np.split(rows["parent"][0], cut), scale_ids=np.split(rows["parent"][1], cut))
        torch.cuda.synchronize()
        assert same(first, old_q), "submit_images() differs from the parent library's sampler and engine"
        print("VTQ_PARENT_LIB: the default sampler's rows and submit_images()'s scores have the parent library's bits")
