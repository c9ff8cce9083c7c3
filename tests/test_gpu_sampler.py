"""Patch coordinates sampled on the GPU: vtq_k_sample_grid (include/vtamiq_hip_sampler.h), vtamiq_amd.sampling and
ImagePairVarlenPipeline.submit_images / submit_group_images.

The contract every test turns on: the kernel's samples have the BITS of the numpy restatement of the header (tests/sampler_model.py, which
tests/test_sampler_model.py holds to the reference's recorded behaviour), a segment's rows depend on nothing but its own table row, key and
the seed, and a pipeline that samples on the device returns the bits of submit() fed with the restatement's coordinates."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sampler_model as SM
from tests.footprint import Arena, arena_bytes
from tests.test_gpu_image_varlen import _direct, _model, same
from tests.test_gpu_streams import Busy
from vtamiq_amd import _lib, sampling
from vtamiq_amd.patches import extract_patches_varlen
from vtamiq_amd.pipeline import ImagePairVarlenPipeline
from vtamiq_amd.validate import average_over_repeats

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
SEED = 2016


def _sample(sizes, counts, keys, seed=SEED, num_scales=1, ratio=1.7, P=16, amount=0.2):
    smp, sid, lengths = sampling.sample_patches(sizes, counts, keys, seed, num_scales, ratio, P,
                                                sampler=sampling.PatchSampler(perturbed_amount=amount), device=DEV)
    torch.cuda.synchronize()
    return smp.cpu().numpy(), (sid.cpu().numpy() if sid is not None else None), lengths


# ---- 1: the bits of the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SM.CATALOGUE, ids=[c.name for c in SM.CATALOGUE])
def test_kernel_has_the_bits_of_the_restatement(case):
    for key in (0, 2 ** 63 + 5):
        got = _sample([case.size], case.count, [key], SEED, case.num_scales, case.ratio, case.P, case.amount)
        want = SM.batch([case.size], case.count, [key], SEED, case.num_scales, case.ratio, case.P, case.amount)
        assert got[0].dtype == np.int32 and got[0].shape == (case.count, 2) and got[2] == want[2] == [case.count]
        assert np.array_equal(got[0], want[0]), (case.name, key, "samples differ from the restatement")
        if case.num_scales > 1:
            assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), (case.name, key, "scale ids")
        else:
            assert got[1] is None and not want[1].any()
    with pytest.raises(ValueError, match="8192"):
        sampling.sample_patches([SM.OVER_LIMIT.size], SM.OVER_LIMIT.count, [0], device=DEV)


# ---- 2: purity -------------------------------------------------------------------------------------------------------------------------------
MIX = [(160, 200), (16, 16), (40, 100), (301, 403), (80, 80), (17, 40), (160, 200)]
MIX_COUNTS = [30, 5, 30, 100, 31, 5, 30]


def test_a_segment_does_not_depend_on_its_batch():
    """An image sampled alone equals the same image inside a batch of seven mixed sizes (one to four levels, 256- and 1024-thread grids in
    one launch when the big image is added) and in reversed order; equal key and size give equal rows; another key or seed does not."""
    keys = [11, 12, 13, 14, 15, 16, 11]                                # image 6 = image 0: key, size and count
    ns = 4
    smp, sid, lengths = _sample(MIX, MIX_COUNTS, keys, num_scales=ns)
    want = SM.batch(MIX, MIX_COUNTS, keys, SEED, ns)
    assert np.array_equal(smp, want[0]) and np.array_equal(sid, want[1]) and lengths == MIX_COUNTS
    cut = np.concatenate([[0], np.cumsum(MIX_COUNTS)])
    rows = lambda a, i: a[cut[i]:cut[i + 1]]
    for i in range(len(MIX)):
        a_smp, a_sid, _ = _sample([MIX[i]], MIX_COUNTS[i], [keys[i]], num_scales=ns)
        assert np.array_equal(a_smp, rows(smp, i)) and np.array_equal(a_sid, rows(sid, i)), i
    r_smp, r_sid, _ = _sample(MIX[::-1], MIX_COUNTS[::-1], keys[::-1], num_scales=ns)
    rcut = np.concatenate([[0], np.cumsum(MIX_COUNTS[::-1])])
    for i in range(len(MIX)):
        j = len(MIX) - 1 - i
        assert np.array_equal(r_smp[rcut[j]:rcut[j + 1]], rows(smp, i)) and np.array_equal(r_sid[rcut[j]:rcut[j + 1]], rows(sid, i)), i
    assert np.array_equal(rows(smp, 0), rows(smp, 6)) and len(np.unique(rows(smp, 0), axis=0)) > 1
    # with a 1024-thread launch geometry (one segment of the batch has more than 256 cells) the small segments keep their rows
    b_smp, _, _ = _sample(MIX + [(64, 128)], MIX_COUNTS + [2049], keys + [17], num_scales=ns)
    assert np.array_equal(b_smp[:cut[-1]], smp)
    other_key, _, _ = _sample([MIX[0]], MIX_COUNTS[0], [keys[0] + 1], num_scales=ns)
    other_seed, _, _ = _sample([MIX[0]], MIX_COUNTS[0], [keys[0]], seed=SEED + 1, num_scales=ns)
    assert not np.array_equal(other_key, rows(smp, 0)) and not np.array_equal(other_seed, rows(smp, 0))
    assert not np.array_equal(other_key, other_seed)


# ---- 3: footprint and refusals of the entry ------------------------------------------------------------------------------------------------
class Entry:
    """vtq_k_sample_grid on a guard-band arena: every table and output has exactly the header's extent."""

    def __init__(self, sizes, counts, num_scales, keys):
        self.plan = sampling.plan_samples(sizes, counts, num_scales)
        self.seg = np.ascontiguousarray(self.plan.seg)
        self.keys = np.ascontiguousarray(np.asarray(keys, np.uint64)[self.plan.seg_image])
        NS, T = len(self.seg), self.plan.total
        specs = [("seg", (NS, 8), I32), ("keys", (NS,), torch.int64), ("samples", (T, 2), I32), ("scale_ids", (T,), I32)]
        self.arena = Arena(arena_bytes([s[1:] for s in specs]), DEV)
        self.b = {name: self.arena.carve(name, shape, dtype) for name, shape, dtype in specs}
        self.b["seg"].copy_(torch.from_numpy(self.seg))
        self.b["keys"].copy_(torch.from_numpy(self.keys.view(np.int64)))
        torch.cuda.synchronize()

    def outputs(self):
        return [self.b["samples"], self.b["scale_ids"]]

    def call(self, **kw):
        b = self.b
        a = dict(seg=b["seg"].data_ptr(), keys=b["keys"].data_ptr(), seg_host=self.seg, keys_host=self.keys, NS=len(self.seg), seed=SEED, q=13107,
                 samples=b["samples"].data_ptr(), scale_ids=b["scale_ids"].data_ptr())
        a.update(kw)
        sh = a["seg_host"].ctypes.data_as(C.POINTER(C.c_int32)) if a["seg_host"] is not None else None
        kh = a["keys_host"].ctypes.data_as(C.POINTER(C.c_uint64)) if a["keys_host"] is not None else None
        lib = _lib.load()
        rc = lib.vtq_k_sample_grid(a["seg"], a["keys"], sh, kh, a["NS"], a["seed"], a["q"], a["samples"], a["scale_ids"],
                                   torch.cuda.current_stream().cuda_stream)
        return rc, lib.vtq_last_error().decode()


def test_entry_footprint():
    """Guards filled with 0x00, then 0xFF: exactly 2 * total and total int32 are written, no guard byte changes, the outputs are
    bit-identical across the fills and equal the restatement.  The sizes cover one to four levels, grids of 1 to 2145 cells in one launch."""
    sizes, counts, keys = MIX + [(64, 128)], MIX_COUNTS + [2049], [21, 22, 23, 24, 25, 26, 27, 28]
    e = Entry(sizes, counts, 4, keys)

    def launch():
        for out in e.outputs():
            e.arena.fill(out, 0xFF)                                   # -1 everywhere: a row the kernel skipped would keep it
        rc, msg = e.call()
        assert rc == 0, msg

    got = e.arena.run_twice(launch, e.outputs)
    want = SM.batch(sizes, counts, keys, SEED, 4)
    assert got[0].shape == (sum(counts), 2) and got[1].shape == (sum(counts),)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def test_level_is_part_of_the_draw_and_refusals_leave_every_buffer_untouched():
    e = Entry([(160, 200)], 30, 1, [5])
    rc, msg = e.call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    level0 = e.b["samples"].cpu().numpy().copy()
    assert np.array_equal(level0, SM.batch([(160, 200)], 30, [5], SEED)[0])
    moved = e.seg.copy()
    moved[0, 6] = 1                                                   # the same grid and extents, drawn as level 1
    dev_moved = torch.from_numpy(moved).to(DEV)
    rc, msg = e.call(seg_host=moved, seg=dev_moved.data_ptr())
    assert rc == 0, msg
    torch.cuda.synchronize()
    level1 = e.b["samples"].cpu().numpy().copy()
    first, n, Hg, Wg, hm, wm, _, _ = e.seg[0].tolist()
    assert np.array_equal(level1, SM.segment(SEED, 5, 1, n, Hg, Wg, hm, wm, 13107).samples) and not np.array_equal(level0, level1)
    assert (e.b["scale_ids"].cpu().numpy() == 1).all()

    e = Entry(MIX, MIX_COUNTS, 4, [1, 2, 3, 4, 5, 6, 7])
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
    cases.update({"NS < 1": dict(NS=0), "n < 1": edit(1, 1, 0), "n > Hg Wg": edit(0, 1, 8000), "Hg Wg > 8192": edit(0, 2, 8192),
                  "negative h - P": edit(0, 4, -1), "level 4": edit(0, 6, 4), "first row": edit(2, 0, 0), "scale_ids NULL with levels": dict(scale_ids=None),
                  "amount_q": dict(q=1 << 16), "seg unaligned": dict(seg=e.b["seg"].data_ptr() + 4)})
    for name, kw in cases.items():
        rc, msg = e.call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_sample_grid:"), (name, rc, msg)
    torch.cuda.synchronize()
    assert e.arena.violations(0x00) == []
    assert torch.equal(e.arena.mem, before), "a refused call wrote to the device"
    rc, msg = e.call()                                                # and the entry still works
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(e.b["samples"].cpu().numpy(), SM.batch(MIX, MIX_COUNTS, [1, 2, 3, 4, 5, 6, 7], SEED, 4)[0])


# ---- 4: end to end -----------------------------------------------------------------------------------------------------------------------
PIPE_SIZES = [(48, 64), (96, 128), (80, 80), (160, 200)]             # one, two, two and three levels when three are asked for


def _images(rs, sizes):
    return [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def _cap(pairs, sizes, count, nscales, repeats=1):
    return dict(max_pairs=pairs * repeats, max_image_bytes=2 * 3 * sum(h * w for h, w in sizes), max_patches=pairs * count * repeats,
                num_scales=nscales)


@pytest.mark.parametrize("nscales,side_stream", [(1, False), (3, False), (3, True)], ids=["1-scale", "3-scales", "3-scales-side-stream"])
def test_submit_images_has_the_bits_of_submit_with_the_restatements_coordinates(nscales, side_stream):
    """Four batches over two slots (the third and fourth reuse one), each another mix of sizes, the third with unaligned sampling and
    pairs of two sizes: submit_images equals submit() fed with the restatement's coordinates for the same keys -- on the same pipeline,
    interleaved, so submit() also keeps its bits beside the new entry (checked against the direct path) -- and a batch over capacity
    is refused with nothing enqueued."""
    m = _model(nscales)
    rs = np.random.RandomState(9)
    count = 40
    mixes = [[0, 1, 2, 3], [3, 3, 0], [1, 2, 0, 3], [2, 0]]
    batches = []
    for it, mix in enumerate(mixes):
        sizes = [PIPE_SIZES[k] for k in mix]
        dsizes = [PIPE_SIZES[(k + 1) % 4] for k in mix] if it == 2 else sizes
        B = len(mix)
        keys = [1000 * it + b for b in range(B)] + ([2 ** 40 + 1000 * it + b for b in range(B)] if it == 2 else [])
        batches.append((_images(rs, sizes), _images(rs, dsizes), sizes, dsizes, keys))

    def run():
        pipe = ImagePairVarlenPipeline(m, **_cap(4, [PIPE_SIZES[3]] * 4, count, nscales))
        got, want = [], []
        for it, (refs, dists, sizes, dsizes, keys) in enumerate(batches):
            aligned = it != 2
            got.append(pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, aligned=aligned))
            smp, sid = SM.per_image(sizes + (dsizes if not aligned else []), count, keys, SEED, nscales)
            want.append(pipe.submit(refs, dists, smp, scale_ids=sid if nscales > 1 else None))
        slot = pipe.count
        with pytest.raises(ValueError, match="images in the batch"):
            pipe.submit_images(batches[0][0] + batches[0][0][:1], batches[0][1] + batches[0][1][:1], count, seed=SEED)
        with pytest.raises(ValueError, match="max_patches"):
            pipe.submit_images(batches[0][0], batches[0][1], count + 1, seed=SEED)
        with pytest.raises(ValueError, match="aligned sampling"):
            pipe.submit_images(batches[2][0], batches[2][1], count, seed=SEED)
        assert pipe.count == slot, "a refused batch took a slot"
        got.append(pipe.submit_images(*batches[0][:2], count, keys=batches[0][4], seed=SEED))     # and the next batch is still right
        return got, want

    if side_stream:
        side, busy = torch.cuda.Stream(), Busy()
        torch.cuda.synchronize()
        busy(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            got, want = run()
    else:
        got, want = run()
    torch.cuda.synchronize()
    for it, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (len(mixes[it]),) and same(g, w), it
    assert same(got[4], got[0]) and not torch.equal(got[0][:2], got[3][:2])
    # submit() itself, on the pipeline that also sampled: the bits of the direct path (per-image extract_patches + forward_varlen)
    refs, dists, sizes, dsizes, keys = batches[2]
    smp, sid = SM.per_image(sizes + dsizes, count, keys, SEED, nscales)
    direct = _direct(m, (refs, dists, smp, sid if nscales > 1 else None), nscales)
    torch.cuda.synchronize()
    assert same(want[2], direct)


@pytest.mark.parametrize("nscales", [1, 3])
def test_submit_group_images_has_the_bits_of_submit_group(nscales):
    m = _model(nscales)
    rs = np.random.RandomState(19)
    rsizes, dsizes = [PIPE_SIZES[0], PIPE_SIZES[3]], [PIPE_SIZES[k] for k in (0, 3, 2, 3, 1)]
    refs, dists, index = _images(rs, rsizes), _images(rs, dsizes), [0, 1, 1, 1, 0]
    keys = [7, 8, 7, 8, 9, 10, 11]                                    # distorted images 0 and 1 share key and size with their reference
    rc, dc = [33, 50], [33, 50, 47, 20, 25]
    cap = dict(max_pairs=4, max_image_bytes=3 * sum(h * w for h, w in rsizes + dsizes), max_patches=sum(dc), num_scales=nscales)
    pipe = ImagePairVarlenPipeline(m, **cap)
    q = pipe.submit_group_images(refs, dists, index, rc, keys=keys, seed=SEED, patch_count_dist=dc)
    smp, sid = SM.per_image(rsizes + dsizes, rc + dc, keys, SEED, nscales)
    assert np.array_equal(smp[0], smp[2]) and np.array_equal(smp[1], smp[3])
    ids = dict(scale_ids_ref=sid[:2], scale_ids_dist=sid[2:]) if nscales > 1 else {}
    want = pipe.submit_group(refs, dists, index, smp[:2], smp[2:], **ids)
    torch.cuda.synchronize()
    assert q.shape == (5,) and same(q, want)
    with pytest.raises(ValueError):
        pipe.submit_group_images(refs, dists, [0, 1, 2, 1, 0], rc, keys=keys, patch_count_dist=dc)
    # repeats: pass r scores distorted image m against reference index[m] of pass r -- the explicit batch of 2 G references and 2 M
    # distorted images, averaged
    big = ImagePairVarlenPipeline(m, **dict(cap, max_pairs=8, max_patches=2 * sum(dc), max_image_bytes=2 * cap["max_image_bytes"]))
    q2 = big.submit_group_images(refs, dists, index, rc, keys=keys, seed=SEED, num_repeats=2, patch_count_dist=dc)
    k2 = [sampling.repeat_key(k, 1) for k in keys]
    smp2, sid2 = SM.per_image(rsizes + dsizes, rc + dc, k2, SEED, nscales)
    ids2 = dict(scale_ids_ref=sid[:2] + sid2[:2], scale_ids_dist=sid[2:] + sid2[2:]) if nscales > 1 else {}
    both = big.submit_group(refs * 2, dists * 2, index + [i + 2 for i in index], smp[:2] + smp2[:2], smp[2:] + smp2[2:], **ids2)
    torch.cuda.synchronize()
    assert both.shape == (10,) and not torch.equal(both[:5], both[5:])
    assert q2.dtype == torch.float64 and q2.shape == (5,) and same(q2, average_over_repeats(both, 2))
    with pytest.raises(ValueError, match="repeats"):
        pipe.submit_group_images(refs, dists, index, rc, keys=keys, num_repeats=2, patch_count_dist=dc)


@pytest.mark.parametrize("nscales", [1, 3])
def test_num_repeats_has_the_bits_of_the_explicit_batch_averaged(nscales):
    """num_repeats=3: the bits of average_over_repeats over the explicit 3B-pair batch (every pair three times, keys repeat_key(key, r)),
    with the images uploaded once: the repeats fit a pipeline whose max_image_bytes holds ONE copy of the images."""
    m = _model(nscales)
    rs = np.random.RandomState(29)
    sizes = [PIPE_SIZES[k] for k in (1, 3, 0)]
    refs, dists, keys, count, R = _images(rs, sizes), _images(rs, sizes), [3, 2 ** 64 - 1, 5], 36, 3
    pipe = ImagePairVarlenPipeline(m, **_cap(3, sizes, count, nscales, repeats=R))
    q = pipe.submit_images(refs, dists, count, keys=keys, seed=SEED, num_repeats=R)
    explicit = ImagePairVarlenPipeline(m, max_pairs=3 * R, max_image_bytes=R * 2 * 3 * sum(h * w for h, w in sizes), max_patches=3 * R * count,
                                       num_scales=nscales)
    keys3 = [sampling.repeat_key(k, r) for r in range(R) for k in keys]
    smp, sid = SM.per_image(sizes * R, count, keys3, SEED, nscales)
    q3 = explicit.submit(refs * R, dists * R, smp, scale_ids=sid if nscales > 1 else None)
    torch.cuda.synchronize()
    assert q3.shape == (9,) and not torch.equal(q3[:3], q3[3:6])
    assert q.dtype == torch.float64 and q.shape == (3,) and same(q, average_over_repeats(q3, R))
    with pytest.raises(ValueError, match="repeats"):
        pipe.submit_images(refs, dists, count, keys=keys, num_repeats=R + 1)


# ---- 5: the existing front end beside the sampler ----------------------------------------------------------------------------------------
def test_extract_patches_varlen_takes_the_sampled_lists_without_a_host_check():
    """sample_patches -> extract_patches_varlen(validate=False): the patches of the same coordinates handed over from the host with the
    range check on (the samples are in range by construction)."""
    rs = np.random.RandomState(3)
    sizes, keys = [(160, 200), (17, 40), (80, 80)], [1, 2, 3]
    images = [torch.from_numpy(im).to(DEV) for im in _images(rs, sizes)]
    smp, sid, lengths = sampling.sample_patches(sizes, 30, keys, SEED, 3, device=DEV)
    got = extract_patches_varlen(images, smp, lengths, sid, 3, validate=False)
    want_smp, want_sid, _ = SM.batch(sizes, 30, keys, SEED, 3)
    want = extract_patches_varlen(images, torch.from_numpy(want_smp), lengths, torch.from_numpy(want_sid), 3, validate=True)
    for g, w in zip(got, want):
        assert same(g, w)
