"""What vtamiq_amd.pipeline and the checking code of vtamiq_amd.patches state once, without a GPU: the word ranges of a slot's int32 block
(block_layout), the slot capacity (block_capacity), the argument checks the entries share, and the range rule of a sample."""
import numpy as np
import pytest
import torch

from vtamiq_amd import sampling
from vtamiq_amd.patches import check_samples_host, check_samples_host_varlen
from vtamiq_amd.pipeline import (ImagePairVarlenPipeline, _host_images, _ref_indices, _sample_lists, block_capacity, block_layout,
                                 pair_arguments, plan_sampled_batch, plan_varlen_batch)

# (NI, T, NS): the batches of test_image_varlen_layout.py and test_sampler_model.py, and one whose tables end off a 4-word boundary
SHAPES = [(4, 200, 12), (2, 80, 6), (12, 360, 24), (4, 120, 8), (5, 77, 7), (1, 1, 1)]


@pytest.mark.parametrize("sampled", [False, True], ids=["host-sampled", "device-sampled"])
@pytest.mark.parametrize("ns", [1, 2, 3, 4])
def test_layout_ranges_are_disjoint_ordered_and_end_at_words(ns, sampled):
    for NI, T, NS in SHAPES:
        L = block_layout(NI, T, NS if sampled else None, ns > 1)
        ranges = [L.tab, L.patch_img, L.seg, L.keys, L.samples, L.ids]
        assert all(r.step is None and 0 <= r.start <= r.stop for r in ranges)
        want = [4 * NI, T, 8 * NS if sampled else 0, 2 * NS if sampled else 0, 2 * T, T if ns > 1 else 0]
        assert [r.stop - r.start for r in ranges] == want
        assert L.tab.start == 0 and L.patch_img.start == L.tab.stop and L.ids.stop == L.words
        for a, b in zip(ranges, ranges[1:]):                          # in the documented order, nothing overlaps ...
            assert a.stop <= b.start
            if b is not L.seg:                                        # ... and nothing but the alignment of seg leaves a gap
                assert a.stop == b.start
        if sampled:
            assert L.seg.start % 4 == 0 and 0 <= L.seg.start - L.patch_img.stop < 4
            assert L.uploaded == L.keys.stop == L.samples.start, "exactly the front is uploaded: the device writes the rest"
        else:
            assert L.seg.start == L.seg.stop == L.patch_img.stop and L.uploaded == L.words, "the whole block is uploaded"
        tab, pimg, seg, keys, smp, sid = L.split(torch.arange(L.words + 3, dtype=torch.int32))
        assert (tab.numel(), pimg.numel(), tuple(seg.shape), keys.numel(), tuple(smp.shape)) == (want[0], T, (want[2] // 8, 8), want[3], (T, 2))
        assert (sid is None) == (ns == 1) and (sid is None or sid.numel() == T)
        assert int(smp[0, 0]) == L.samples.start and int(pimg[0]) == 4 * NI
    assert block_layout(5, 77, 7).seg.start == 100 and block_layout(5, 77).samples.start == 97


# what the commit before this module's layout function computed for these batches, recorded from a run of its plan functions
VARLEN_WORDS = {1: (616, 248), 2: (816, 328), 3: (816, 328), 4: (816, 328)}
SAMPLED = {1: ((12, 408, 528, 1248), (4, 136, 176, 416)), 2: ((18, 408, 588, 1668), (6, 136, 196, 556)),
           3: ((24, 408, 648, 1728), (8, 136, 216, 576)), 4: ((24, 408, 648, 1728), (8, 136, 216, 576))}


@pytest.mark.parametrize("ns", [1, 2, 3, 4])
def test_planned_batches_keep_their_recorded_offsets(ns):
    cap = dict(max_images=4, max_image_bytes=3 * (48 * 64 + 96 * 128) * 2, max_patches=100, num_scales=ns)
    two = plan_varlen_batch([(48, 64), (96, 128)], [(48, 64), (96, 128)], [40, 60], [40, 60], **cap)
    one = plan_varlen_batch([(48, 64)], [(48, 64)], [40], [40], **cap)
    assert (two.words, one.words) == VARLEN_WORDS[ns]
    L = block_layout(4, 200, None, ns > 1)
    assert (L.samples.start, L.ids.start, L.words) == (4 * 4 + 200, 4 * 4 + 3 * 200, two.words)
    sizes = [(48, 64), (160, 200)]
    cap = dict(max_images=12, max_image_bytes=2 * 3 * (48 * 64 + 160 * 200), max_patches=180, num_scales=ns)
    three = plan_sampled_batch(sizes, sizes, [30, 30], [30, 30], [5, 6], [5, 6], repeats=3, **cap)
    single = plan_sampled_batch(sizes, sizes[::-1], [30, 30], [30, 30], [5, 6], [7, 8], **cap)
    for sb, want in zip((three, single), SAMPLED[ns]):
        assert (len(sb.seg), sb.seg_at, sb.front, sb.batch.words) == want
        L = block_layout(len(sb.batch.sizes), sb.batch.tables.total, len(sb.seg), ns > 1)
        assert (L.seg.start, L.uploaded, L.words) == want[1:]
        assert L.keys.start == sb.seg_at + 8 * len(sb.seg) and L.samples.start == sb.front


@pytest.mark.parametrize("max_pairs,max_patches", [(3, 111), (4, 240), (1, 9)])
@pytest.mark.parametrize("ns", [1, 2, 3, 4])
def test_a_batch_at_the_caps_fits_the_block_and_one_image_more_is_refused_by_the_plan(ns, max_pairs, max_patches):
    MI = 2 * max_pairs
    words = block_capacity(MI, max_patches, ns)
    assert words >= 4 * MI + 2 * max_patches * (4 if ns > 1 else 3) + 10 * ns * MI + 4, "never smaller than the size slots had before"
    sizes, counts = [(64, 64)] * max_pairs, [max_patches // max_pairs] * max_pairs
    cap = dict(max_images=MI, max_image_bytes=MI * 3 * 64 * 64, max_patches=max_patches, num_scales=ns)
    sb = plan_sampled_batch(sizes, sizes, counts, counts, list(range(max_pairs)), list(range(max_pairs)), repeats=1, **cap)
    assert len(sb.batch.sizes) == MI and sb.batch.words <= words and sb.front <= sb.batch.words
    assert len(sb.seg) == MI * min(ns, sampling.compute_patch_num_scales(ns, 64, 64, 16, 16))
    host = plan_varlen_batch(sizes, sizes, counts, counts, **cap)
    assert host.words <= sb.batch.words <= words
    # the worst case within the caps: every patch allowed, one segment per image and level
    worst = block_layout(MI, 2 * max_patches, ns * MI, ns > 1)
    assert worst.words <= words
    parts = worst.split(torch.zeros(words, dtype=torch.int32))
    assert parts[4].shape == (2 * max_patches, 2) and (parts[5] is None or parts[5].numel() == 2 * max_patches)
    more = sizes + [(64, 64)]
    with pytest.raises(ValueError, match="images in the batch"):
        plan_sampled_batch(more, sizes, counts + [1], counts, list(range(max_pairs + 1)), list(range(max_pairs)), **cap)
    with pytest.raises(ValueError, match="images in the batch"):
        plan_varlen_batch(more, sizes, counts + [1], counts, **cap)


# ---- the checks the entries share ----------------------------------------------------------------------------------------------------------
def _bare(ns=1):
    """An ImagePairVarlenPipeline without a device: what its entries read before they touch a slot.  An entry that got past its argument
    checks would fail on the missing ring with an AttributeError, not with the ValueError asked for."""
    p = object.__new__(ImagePairVarlenPipeline)
    p.num_scales, p.P, p.count, p.depth, p._batch = ns, 16, 0, 2, None
    p.max_images, p.max_image_bytes, p.max_patches = 8, 8 * 3 * 64 * 64, 200
    p._caps = dict(max_images=8, max_image_bytes=p.max_image_bytes, max_patches=200, num_scales=ns, patch_size=16)
    return p


def _img(h=48, w=64, c=3, dtype=np.uint8):
    return np.zeros((h, w, c), dtype)


def _smp(n=20):
    return np.zeros((n, 2), np.int32)


BAD_IMAGES = {"float image": lambda: ([_img(dtype=np.float32)], [_img()]), "four channels": lambda: ([_img()], [_img(c=4)]),
              "no references": lambda: ([], [_img()]), "no distorted images": lambda: ([_img()], [])}


@pytest.mark.parametrize("case", list(BAD_IMAGES))
def test_every_entry_refuses_the_same_images(case):
    refs, dists = BAD_IMAGES[case]()
    n = max(len(refs), len(dists))
    p = _bare()
    for pairs in (False, True):
        with pytest.raises(ValueError):
            _host_images(refs, dists, pairs=pairs)
    with pytest.raises(ValueError):
        pair_arguments(refs, dists, [_smp()] * n)
    with pytest.raises(ValueError):
        p.submit(refs, dists, [_smp()] * n)
    with pytest.raises(ValueError):
        p.submit_group(refs, dists, [0] * len(dists), [_smp()] * len(refs), [_smp()] * len(dists))
    with pytest.raises(ValueError):
        p.submit_images(refs, dists, 20, keys=list(range(n)))
    with pytest.raises(ValueError):
        p.submit_group_images(refs, dists, [0] * len(dists), 20, keys=list(range(len(refs) + len(dists))))
    assert p.count == 0 and p._batch is None


@pytest.mark.parametrize("index", [[0, 2], [0, -1], [0], [0, 1, 0]], ids=["past G", "negative", "too short", "too long"])
def test_every_group_entry_refuses_the_same_ref_index(index):
    refs, dists = [_img(), _img(80, 80)], [_img(), _img(80, 80)]
    p = _bare()
    with pytest.raises(ValueError, match="ref_index"):
        _ref_indices(index, 2, 2)
    with pytest.raises(ValueError, match="ref_index"):
        p.submit_group(refs, dists, index, [_smp(), _smp()], [_smp(), _smp()])
    with pytest.raises(ValueError, match="ref_index"):
        p.submit_group_images(refs, dists, index, 20, keys=[1, 2, 3, 4])
    p._batch = p.plan([(48, 64), (80, 80)], [(48, 64), (80, 80)], [20, 20], [20, 20])           # as acquire() leaves it
    with pytest.raises(ValueError, match="ref_index"):
        p.launch_group(index)
    assert p.count == 0 and _ref_indices([1, 0], 2, 2) == [1, 0]


def test_every_entry_refuses_scale_ids_and_patch_counts_of_the_wrong_length():
    refs, dists = [_img(), _img(80, 80)], [_img(), _img(80, 80)]
    ids = lambda n=20: np.zeros(n, np.int32)
    p = _bare(2)
    with pytest.raises(ValueError, match="scale_ids"):
        _sample_lists([_smp(), _smp()], [ids(), ids(19)], 2)
    with pytest.raises(ValueError, match="scale_ids"):
        _sample_lists([_smp(), _smp()], [ids()], 2)
    with pytest.raises(ValueError, match="scale_ids"):
        _sample_lists([_smp()], None, 2)
    assert _sample_lists([_smp()], [ids(19)], 1)[1] is None           # one level: ids are not read
    with pytest.raises(ValueError, match="scale_ids"):
        pair_arguments(refs, dists, [_smp(), _smp()], scale_ids=[ids(), ids(19)], num_scales=2)
    with pytest.raises(ValueError, match="scale_ids"):
        p.submit(refs, dists, [_smp(), _smp()], scale_ids=[ids(), ids(19)])
    with pytest.raises(ValueError, match="scale_ids"):
        p.submit(refs, dists, [_smp(), _smp()], scale_ids=[ids()] * 3)
    with pytest.raises(ValueError, match="scale_ids"):
        p.submit_group(refs, dists, [0, 1], [_smp(), _smp()], [_smp(), _smp()], scale_ids_ref=[ids(), ids()], scale_ids_dist=[ids(), ids(21)])
    with pytest.raises(ValueError, match="scale_ids"):
        p.submit_group(refs, dists, [0, 1], [_smp(), _smp()], [_smp(), _smp()], scale_ids_ref=[ids(), ids()])
    for bad in ([20], [20, 20, 20]):
        with pytest.raises(ValueError, match="patch_count"):
            sampling.patch_counts(bad, 2)
        with pytest.raises(ValueError, match="patch_count"):
            sampling.plan_samples([(48, 64), (80, 80)], bad, 2)
        with pytest.raises(ValueError, match="patch_count"):
            p.submit_images(refs, dists, bad, keys=[1, 2])
        with pytest.raises(ValueError, match="patch_count"):
            p.submit_group_images(refs, dists, [0, 1], bad, keys=[1, 2, 3, 4], patch_count_dist=[20, 20])
        with pytest.raises(ValueError, match="patch_count"):
            p.submit_group_images(refs, dists, [0, 1], [20, 20], keys=[1, 2, 3, 4], patch_count_dist=bad)
    assert sampling.patch_counts(7, 3) == [7, 7, 7] and sampling.patch_counts(np.array([3, 4]), 2) == [3, 4]
    assert p.count == 0 and p._batch is None


# ---- the range rule ------------------------------------------------------------------------------------------------------------------------
def _raises_index_error(fn):
    try:
        fn()
    except IndexError:
        return True
    return False


@pytest.mark.parametrize("H,W,P", [(48, 64, 16), (40, 24, 8)])
@pytest.mark.parametrize("ns", [1, 3, 4])
def test_both_range_checks_state_one_rule(H, W, P, ns):
    """check_samples_host on host tensors [NI, N, 2] and check_samples_host_varlen on the same samples laid out per image agree at the
    corners of every level, one step past them, and on scale ids outside [0, num_scales) -- and with the rule written out here."""
    def both(r, c, s):
        smp = np.zeros((2, 3, 2), np.int32)                           # two images of one size, three samples each: the probe is the last
        sid = np.zeros((2, 3), np.int32)
        smp[1, 2], sid[1, 2] = (r, c), s
        ids = (torch.from_numpy(sid), sid.reshape(-1)) if ns > 1 else (None, None)
        a = _raises_index_error(lambda: check_samples_host(torch.from_numpy(smp), ids[0], H, W, ns, P))
        b = _raises_index_error(lambda: check_samples_host_varlen(smp.reshape(-1, 2), ids[1], [(H, W)] * 2, [3, 3], ns, P))
        assert a == b, (r, c, s, a, b)
        return a

    for s in range(ns):
        h, w = H >> s, W >> s
        for r, c in ((0, 0), (h - P, w - P), (h - P + 1, 0), (0, w - P + 1), (-1, 0)):
            inside = 0 <= r <= h - P and 0 <= c <= w - P
            assert both(r, c, s) == (not inside), (s, r, c)
    if ns > 1:
        assert both(0, 0, -1) and both(0, 0, ns) and not both(0, 0, 0)
    assert (H >> 2) < P or (W >> 2) < P, "level 2 of these images holds no patch: every sample on it is refused"
