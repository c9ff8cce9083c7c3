"""Host side of the image front end for images of different sizes (vtamiq_amd.patches.image_tables / check_samples_host_varlen, the
argument checking of vtamiq_amd.pipeline.ImagePairVarlenPipeline): no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import image_varlen_cases as IC
from vtamiq_amd import _lib
from vtamiq_amd.patches import check_samples_host_varlen, image_tables
from vtamiq_amd.pipeline import pair_arguments, plan_varlen_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (17, 33), (37, 53), (64, 67)]


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (1, 0, 3, 2), (3, 2, 1, 0), (1, 1, 2, 0)])
def test_tables_are_exact_byte_sums_prefixes_and_patch_maps(order):
    sizes = [SIZES[i] for i in order]
    lengths = [[1, 2, 5, 9][i] for i in order]
    t = image_tables(sizes, lengths)
    off, row = 0, 0
    for i, ((h, w), n) in enumerate(zip(sizes, lengths)):
        assert t.img_off[i] == off and t.row0[i] == row and (t.H[i], t.W[i]) == (h, w)
        assert (int(t.tab[i, 0]) & 0xffffffff) | (int(t.tab[i, 1]) << 32) == off and tuple(t.tab[i, 2:]) == (h, w)
        assert (t.patch_img[row:row + n] == i).all()
        off, row = off + 3 * h * w, row + n
    assert t.image_bytes == off and t.total == row == t.row0[-1] == len(t.patch_img)
    assert t.img_off.dtype == np.int64 and all(a.dtype == np.int32 for a in (t.H, t.W, t.row0, t.tab, t.patch_img))
    assert any(o % 2 for o in t.img_off), "17 x 33 x 3 = 1683 bytes: an image behind it starts at an odd byte"


def test_tables_take_empty_images_and_offsets_past_32_bits():
    t = image_tables([(16, 16), (20, 20), (16, 16)], [3, 0, 2])
    assert t.row0.tolist() == [0, 3, 3, 5] and t.patch_img.tolist() == [0, 0, 0, 2, 2]
    big = image_tables([(40000, 40000), (16, 16)], [1, 1])           # 4.8e9 bytes in front of the second image: both table words are used
    assert big.img_off[1] == 3 * 40000 * 40000 > 2 ** 32
    lo, hi = int(big.tab[1, 0]) & 0xffffffff, int(big.tab[1, 1])
    assert lo | (hi << 32) == big.img_off[1] and hi == 1
    with pytest.raises(ValueError):
        image_tables([(16, 16)], [1, 2])                             # one count per image
    with pytest.raises(ValueError):
        image_tables([(16, 0)], [1])
    with pytest.raises(ValueError):
        image_tables([], [])
    with pytest.raises(ValueError):
        image_tables([(16, 16)], [-1])
    with pytest.raises(ValueError):
        image_tables([(16, 16)], [1.0])


@pytest.mark.parametrize("P", [16, 8])
def test_case_samples_reach_every_corner_of_every_level_and_every_flip(P):
    """The shared GPU cases: over ROUNDS turns every image has had a patch at each corner of each level that holds one, and all four flips."""
    seen = [set() for _ in IC.SIZES]
    flips = [set() for _ in IC.SIZES]
    for turn in range(IC.ROUNDS):
        smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, IC.NUM_SCALES, P, 7, turn)
        check_samples_host_varlen(np.concatenate(smp), np.concatenate(sid), IC.SIZES, IC.COUNTS, IC.NUM_SCALES, P)
        for k, (a, s) in enumerate(zip(smp, sid)):
            assert a.shape == (IC.COUNTS[k], 2) and a.dtype == np.int32
            seen[k] |= {(int(r), int(c), int(l)) for (r, c), l in zip(a, s)}
            flips[k].add(IC.flips_of_turn(len(IC.SIZES), turn)[k])
    for k, (h, w) in enumerate(IC.SIZES):
        want = {(r, c, s) for s in IC.levels_with_a_patch(h, w, IC.NUM_SCALES, P) for r, c in IC.corners(h, w, s, P)}
        assert want <= seen[k], (k, want - seen[k])
        assert len(flips[k]) == 4
    if P == 16:
        assert IC.levels_with_a_patch(16, 16, 3, P) == [0] and IC.corners(16, 16, 0, P) == [(0, 0)]
        assert IC.levels_with_a_patch(64, 67, 3, P) == [0, 1, 2] and IC.corners(64, 67, 2, P) == [(0, 0)]
        assert IC.levels_with_a_patch(37, 53, 3, P) == [0, 1] and (37 >> 1, 53 >> 1) == (18, 26)


@pytest.mark.parametrize("P", [16, 8])
def test_range_check_accepts_every_corner_and_rejects_one_past_it(P):
    sizes, ns = SIZES, 3
    for k, (h, w) in enumerate(sizes):
        lengths = [0] * len(sizes)
        lengths[k] = 1
        for s in IC.levels_with_a_patch(h, w, ns, P):
            hm, wm = (h >> s) - P, (w >> s) - P
            for r, c in IC.corners(h, w, s, P):
                check_samples_host_varlen(np.array([[r, c]], np.int32), np.array([s], np.int32), sizes, lengths, ns, P)
            for r, c in ((-1, 0), (0, -1), (hm + 1, 0), (0, wm + 1), (hm + 1, wm + 1), (hm, wm + 1), (hm + 1, wm)):
                with pytest.raises(IndexError):
                    check_samples_host_varlen(np.array([[r, c]], np.int32), np.array([s], np.int32), sizes, lengths, ns, P)
        for s in set(range(ns)) - set(IC.levels_with_a_patch(h, w, ns, P)):          # a level of THIS image smaller than a patch
            with pytest.raises(IndexError):
                check_samples_host_varlen(np.array([[0, 0]], np.int32), np.array([s], np.int32), sizes, lengths, ns, P)


def test_range_check_is_per_image_and_rejects_bad_scale_ids():
    sizes, lengths = [(16, 16), (64, 67)], [1, 2]
    ok = np.array([[0, 0], [48, 51], [16, 17]], np.int32)
    sid = np.array([0, 0, 1], np.int32)
    check_samples_host_varlen(ok, sid, sizes, lengths, 3, 16)
    check_samples_host_varlen(torch.from_numpy(ok).numpy(), sid, sizes, np.array(lengths), 3, 16)
    swapped = ok[[1, 0, 2]]                                          # (48, 51) is inside 64 x 67 and outside 16 x 16
    with pytest.raises(IndexError):
        check_samples_host_varlen(swapped, sid, sizes, lengths, 3, 16)
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            check_samples_host_varlen(ok, np.array([0, 0, bad], np.int32), sizes, lengths, 3, 16)
    with pytest.raises(IndexError):                                  # level 1 of the 16 x 16 image is 8 x 8: smaller than the patch
        check_samples_host_varlen(ok, np.array([1, 0, 1], np.int32), sizes, lengths, 3, 16)
    with pytest.raises(ValueError):
        check_samples_host_varlen(ok, None, sizes, lengths, 3, 16)   # scale ids are required with levels
    with pytest.raises(ValueError):
        check_samples_host_varlen(ok[:2], None, sizes, lengths, 1, 16)
    with pytest.raises(ValueError):
        check_samples_host_varlen(ok, sid, sizes, lengths, 5, 16)
    check_samples_host_varlen(ok[[0, 2, 2]], None, sizes, lengths, 1, 16)          # one level: no ids needed


def test_pipeline_capacity_and_aligned_size_errors_without_a_device():
    cap = dict(max_images=4, max_image_bytes=3 * (48 * 64 + 96 * 128) * 2, max_patches=100)
    b = plan_varlen_batch([(48, 64), (96, 128)], [(48, 64), (96, 128)], [40, 60], [40, 60], **cap)
    assert b.n_first == 2 and b.tables.total == 200 and b.tables.image_bytes == cap["max_image_bytes"] and b.words == 4 * 4 + 3 * 200
    assert plan_varlen_batch([(48, 64)], [(48, 64)], [40], [40], num_scales=2, **cap).words == 4 * 2 + 4 * 80
    with pytest.raises(ValueError, match="images in the batch"):
        plan_varlen_batch([(16, 16)] * 3, [(16, 16)] * 3, [1] * 3, [1] * 3, **cap)
    with pytest.raises(ValueError, match="max_patches"):
        plan_varlen_batch([(48, 64), (96, 128)], [(48, 64), (96, 128)], [41, 60], [41, 60], **cap)
    with pytest.raises(ValueError, match="max_image_bytes"):
        plan_varlen_batch([(48, 64), (96, 129)], [(48, 64), (96, 128)], [40, 60], [40, 60], **cap)
    with pytest.raises(ValueError, match="smaller than one"):
        plan_varlen_batch([(15, 64)], [(48, 64)], [4], [4], **cap)
    with pytest.raises(ValueError, match="at least one patch"):
        plan_varlen_batch([(48, 64)], [(48, 64)], [0], [4], **cap)
    with pytest.raises(ValueError):
        plan_varlen_batch([], [(48, 64)], [], [4], **cap)

    img = lambda h, w: np.zeros((h, w, 3), np.uint8)
    smp = lambda n: np.zeros((n, 2), np.int32)
    refs, dists, s2, sid, lens = pair_arguments([img(48, 64), img(80, 80)], [img(48, 64), img(80, 80)], [smp(20), smp(30)])
    assert lens == [20, 30] and len(s2) == 4 and s2[2] is s2[0] and sid is None
    with pytest.raises(ValueError, match="aligned sampling"):
        pair_arguments([img(48, 64)], [img(64, 48)], [smp(20)])
    assert pair_arguments([img(48, 64)], [img(64, 48)], [smp(20), smp(20)])[4] == [20]          # unaligned sampling: any two sizes
    with pytest.raises(ValueError, match="same patch count"):
        pair_arguments([img(48, 64)], [img(64, 48)], [smp(20), smp(21)])
    with pytest.raises(ValueError, match="lengths"):
        pair_arguments([img(48, 64)], [img(48, 64)], [smp(20)], lengths=[21])
    with pytest.raises(ValueError, match="scale_ids"):
        pair_arguments([img(48, 64)], [img(48, 64)], [smp(20)], num_scales=2)
    with pytest.raises(ValueError):
        pair_arguments([img(48, 64)], [img(48, 64)], [smp(20)], scale_ids=[np.zeros(19, np.int32)], num_scales=2)
    with pytest.raises(ValueError):
        pair_arguments([img(48, 64).astype(np.float32)], [img(48, 64)], [smp(20)])
    with pytest.raises(ValueError):
        pair_arguments([img(48, 64)], [img(48, 64)], [smp(20)] * 3)


def test_oracle_composition_commutes_with_a_permutation_of_the_images():
    P = 16
    images = IC.make_images(IC.SIZES, 3)
    smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, IC.NUM_SCALES, P, 7)
    flips = IC.flips_of_turn(len(images), 1)
    pa, po, sc = IC.oracle_batch(images, smp, sid, IC.NUM_SCALES, flips, P)
    assert pa.shape == (sum(IC.COUNTS), 3, P, P) and po.shape == (sum(IC.COUNTS), 2) and sc.shape == (sum(IC.COUNTS),)
    perm = [3, 0, 4, 2, 1]
    pick = lambda x: [x[i] for i in perm]
    pa2, po2, sc2 = IC.oracle_batch(pick(images), pick(smp), pick(sid), IC.NUM_SCALES, pick(flips), P)
    row0 = np.concatenate([[0], np.cumsum(IC.COUNTS)])
    rows = np.concatenate([np.arange(row0[i], row0[i + 1]) for i in perm])
    assert torch.equal(pa2, pa[rows]) and torch.equal(po2, po[rows]) and torch.equal(sc2, sc[rows])
    # the composition is the oracle's own order for one image with one level list
    one = IC.oracle_image(images[4], smp[4], np.zeros_like(sid[4]), 1, (0, 0), P)
    from oracle import patch_oracle as PO
    ref = PO.extract_patches([PO.transform_img(images[4])], [[smp[4].T.astype(np.int64)]], P)
    assert torch.equal(one[0], ref[0][0]) and torch.equal(one[1], ref[1][0]) and one[2] is None


def test_images_header_declares_exactly_the_bound_entry_and_the_library_exports_it():
    from vtamiq_amd import build
    header = open(os.path.join(ROOT, "include", "vtamiq_hip_images.h")).read()
    declared = set(re.findall(r"\b(vtq_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.IMAGE_SIGNATURES) == {"vtq_k_gather_patches_u8"}
    main = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    assert "vtq_k_gather_patches_u8" not in main
    assert not set(_lib.IMAGE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.ROLLOUT_SIGNATURES) | set(_lib.FP8_SIGNATURES))
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "vtq_k_gather_patches_u8")
    lib.vtq_abi_version.restype = ctypes.c_int
    assert lib.vtq_abi_version() == _lib.ABI_VERSION == 10
    nargs = len(re.search(r"vtq_k_gather_patches_u8\((.*?)\);", header, re.S).group(1).split(","))
    assert nargs == len(_lib.IMAGE_SIGNATURES["vtq_k_gather_patches_u8"][1])


def test_entry_refuses_bad_arguments_without_a_device():
    """Every refusal of include/vtamiq_hip_images.h is decided on HOST arrays before any HIP call: they can be provoked here, with made-up
    device addresses that are never dereferenced."""
    lib = _lib.load()
    t = image_tables([(16, 16), (17, 33)], [1, 2])
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ptr = lambda a, ty: a.ctypes.data_as(ctypes.POINTER(ty))
    DEV = 0x10000                                                    # stands for a device address: non-NULL, 16-byte aligned

    def call(**kw):
        a = dict(images=DEV, image_bytes=t.image_bytes, tab=DEV, patch_img=DEV, img_off=t.img_off, H=t.H, W=t.W, row0=t.row0, NI=2, samples=DEV,
                 scale_ids=None, flips=None, mean=f3, std=f3, patches=DEV, pos=DEV, scales=None, P=16, ns=1)
        a.update(kw)
        host = lambda k, ty: ptr(a[k], ty) if a[k] is not None else None
        rc = lib.vtq_k_gather_patches_u8(a["images"], a["image_bytes"], a["tab"], a["patch_img"], host("img_off", ctypes.c_int64),
                                         host("H", ctypes.c_int32), host("W", ctypes.c_int32), host("row0", ctypes.c_int32), a["NI"],
                                         a["samples"], a["scale_ids"], a["flips"], a["mean"], a["std"], a["patches"], a["pos"], a["scales"],
                                         a["P"], a["ns"], None)
        return rc, lib.vtq_last_error().decode()

    i32 = lambda *v: np.array(v, np.int32)
    cases = {k: {k: None} for k in ("images", "tab", "patch_img", "img_off", "H", "W", "row0", "samples", "mean", "std", "patches", "pos")}
    cases.update({
        "NI < 1": dict(NI=0), "row0 decreases": dict(row0=i32(0, 2, 1)), "row0[0] != 0": dict(row0=i32(1, 2, 3)),
        "no patches": dict(row0=i32(0, 0, 0)), "P": dict(P=12), "num_scales 0": dict(ns=0), "num_scales 5": dict(ns=5, scale_ids=DEV),
        "scale_ids NULL": dict(ns=2), "image smaller than P": dict(H=i32(15, 17)), "P = 16 on an 8-row image": dict(H=i32(8, 17)),
        "image leaves the buffer": dict(image_bytes=t.image_bytes - 1), "negative offset": dict(img_off=np.array([-1, 768], np.int64)),
        "tab unaligned": dict(tab=DEV + 4)})
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_gather_patches_u8:"), (name, rc, msg)
