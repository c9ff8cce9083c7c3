"""The device sampler without a device: its numpy restatement (tests/sampler_model.py) against the structure and the statistics of the
reference's default sampler (tests/golden/sampler_reference.npz, recorded by tests/golden/make_sampler_golden.py), the host arithmetic of
vtamiq_amd.sampling against the reference's recorded table, the Python layer's refusals and the refusals of vtq_k_sample_grid.

The statistical conditions are derived, not tuned.  Over K keys, a cell's occupancy is Binomial(K, n / M): it must lie within 5 sigma of
K n / M.  An in-cell offset is uniform on 0.5 +- 2 a, standard deviation 4 a / sqrt(12): the mean of S of them must lie within
5 (4 a / sqrt 12) / sqrt(S) of 0.5.  The recorded reference meets both, and so must the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import sampler_model as SM
from vtamiq_amd import _lib, sampling
from vtamiq_amd.patches import check_samples_host_varlen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sampler_reference.npz"))
SEED = 2016


def _ids(cases):
    return [c.name for c in cases]


# ---- structure, on the whole catalogue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SM.CATALOGUE, ids=_ids(SM.CATALOGUE))
def test_catalogue_case_has_the_reference_structure(case):
    tab = SM.case_table(case)
    assert [(s, n, Hg, Wg) for _, _, n, Hg, Wg, _, _, s in tab] == case.expect, "the case is no longer the edge its name says"
    assert sum(n for _, _, n, *_ in tab) == case.count
    a, P = case.amount, case.P
    for key in (0, 1, 2 ** 63 + 5):
        rows, ids = [], []
        for (_, first, n, Hg, Wg, hm, wm, s), seg in zip(tab, SM.case_segments(case, SEED, key)):
            assert first == len(np.concatenate(rows)) if rows else first == 0
            G = np.array([Hg, Wg], np.int64)
            # the cell of every sample, recovered from the integer t: distinct pairs, inside the grid
            cell = (seg.t - seg.jitter - (1 << 23)) >> 24
            assert ((cell << 24) + (1 << 23) + seg.jitter == seg.t).all() and (cell == seg.cells).all()
            assert (cell >= 0).all() and (cell < G).all() and len({tuple(c) for c in cell.tolist()}) == n
            if a <= 0.25:
                assert ((seg.t >> 24) == cell).all()                  # the jitter stays inside the cell: t alone names it
            off = (seg.t - (cell << 24)) / float(1 << 24)
            assert (off >= 0.5 - 2 * a).all() and (off <= 0.5 + 2 * a).all()
            if a == 0:
                assert (seg.jitter == 0).all()
            # the integer sample is the truncated real one
            real = np.clip(seg.t / float(1 << 24) / G, 0.0, 1.0) * np.array([hm, wm])
            assert (np.abs(seg.samples - np.floor(real)) <= 1).all() and (seg.samples <= real + 1e-6).all()
            assert seg.samples.dtype == np.int32 and seg.samples.shape == (n, 2)
            rows.append(seg.samples), ids.append(np.full(n, s, np.int32))
        smp, sid = np.concatenate(rows), np.concatenate(ids)
        check_samples_host_varlen(smp, sid if case.num_scales > 1 else None, [case.size], [case.count], case.num_scales, P)
        got = SM.batch([case.size], case.count, [key], SEED, case.num_scales, case.ratio, P, a)
        assert np.array_equal(got[0], smp) and np.array_equal(got[1], sid) and got[2] == [case.count]
    if case.size == (P, P):
        assert not smp.any()


def test_catalogue_reaches_the_clamp_and_the_far_edge():
    """amount 0.5 moves a border cell's sample across the grid's edge (t is clamped there) and the far edge dim - P is reached."""
    case = next(c for c in SM.CATALOGUE if c.name.startswith("amount 0.5: jitter"))
    low = high = edge = False
    for key in range(200):
        (_, _, n, Hg, Wg, hm, wm, _), = SM.case_table(case)
        seg, = SM.case_segments(case, SEED, key)
        G = np.array([Hg, Wg], np.int64) << 24
        low, high = low or bool((seg.t < 0).any()), high or bool((seg.t > G).any())
        edge = edge or bool((seg.samples == np.array([hm, wm])).any())
    assert low and high and edge


def test_a_segment_depends_on_seed_key_and_level_only():
    base = SM.segment(1, 2, 0, 40, 6, 8, 80, 112, 13107).samples
    assert np.array_equal(base, SM.segment(1, 2, 0, 40, 6, 8, 80, 112, 13107).samples)
    for other in ((3, 2, 0), (1, 3, 0), (1, 2, 1), (1, 2 + 2 ** 32, 0), (1 + 2 ** 32, 2, 0)):
        assert not np.array_equal(base, SM.segment(*other, 40, 6, 8, 80, 112, 13107).samples), other
    assert np.array_equal(SM.rng(-1, -1, 0, 0, [5]), SM.rng(2 ** 64 - 1, 2 ** 64 - 1, 0, 0, [5]))


def test_rng_is_murmurhash3_x86_32():
    """Against a scalar transcription of the published algorithm on Python ints, and its published test vectors for whole 4-byte blocks
    (seed 0: the empty message -> 0; the bytes 21 43 65 87 -> 0xf55b516b; four zero bytes -> 0x2362f9de)."""
    def mm3(words):
        h = 0
        for k in words:
            k = (k * 0xcc9e2d51) & 0xffffffff
            k = ((k << 15) | (k >> 17)) & 0xffffffff
            k = (k * 0x1b873593) & 0xffffffff
            h ^= k
            h = ((h << 13) | (h >> 19)) & 0xffffffff
            h = (h * 5 + 0xe6546b64) & 0xffffffff
        h ^= 4 * len(words)
        h ^= h >> 16
        h = (h * 0x85ebca6b) & 0xffffffff
        h ^= h >> 13
        h = (h * 0xc2b2ae35) & 0xffffffff
        return h ^ (h >> 16)

    assert mm3([]) == 0 and mm3([0x87654321]) == 0xf55b516b and mm3([0]) == 0x2362f9de
    for seed, key, level, purpose in ((0, 0, 0, 0), (SEED, 0x0123456789abcdef, 3, 2), (2 ** 64 - 1, 2 ** 63, 1, 1)):
        idx = [0, 1, 255, 8191, 2 ** 31]
        want = [mm3([seed & 0xffffffff, seed >> 32, key & 0xffffffff, key >> 32, level, purpose, i]) for i in idx]
        assert SM.rng(seed, key, level, purpose, idx).tolist() == want


# ---- statistics: the recorded reference and the restatement under the same derived conditions -----------------------------------------------
def _occupancy_ok(occ, K, n):
    M = occ.size
    p = n / M
    sigma = np.sqrt(K * p * (1 - p))
    worst = np.abs(occ - K * p).max()
    return worst <= 5 * sigma, worst / sigma if sigma else 0.0


def _offset_ok(offset_sum, S, a):
    bound = 5 * (4 * a / np.sqrt(12)) / np.sqrt(S)
    worst = np.abs(np.asarray(offset_sum) / S - 0.5).max()
    return worst <= bound, worst, bound


@pytest.mark.parametrize("i", range(len(GOLD["shapes"])))
def test_reference_and_restatement_meet_the_same_statistical_conditions(i):
    h, w, n = GOLD["shapes"][i].tolist()
    K, P = int(GOLD["K"]), int(GOLD["P"])
    Hg, Wg = GOLD[f"grid_{i}"].tolist()
    assert (Hg, Wg) == SM.grid(n, h, w) == sampling.grid_dims(n, h, w)
    # the reference, as recorded
    occ = GOLD[f"occupancy_{i}"]
    assert occ.shape == (Hg, Wg) and occ.sum() == K * n
    ok, z = _occupancy_ok(occ, K, n)
    assert ok, f"reference occupancy {z:.2f} sigma"
    ok, worst, bound = _offset_ok(GOLD[f"offset_sum_{i}"], K * n, 0.2)
    assert ok, (worst, bound)
    # the restatement, K keys
    occ2, off2 = np.zeros((Hg, Wg), np.int64), np.zeros(2)
    for key in range(K):
        seg = SM.segment(SEED, key, 0, n, Hg, Wg, h - P, w - P, SM.amount_q(0.2))
        np.add.at(occ2, (seg.cells[:, 0], seg.cells[:, 1]), 1)
        off2 += ((seg.t - (seg.cells << 24)) / float(1 << 24)).sum(axis=0)
    ok, z = _occupancy_ok(occ2, K, n)
    assert ok, f"restatement occupancy {z:.2f} sigma"
    ok, worst, bound = _offset_ok(off2, K * n, 0.2)
    assert ok, (worst, bound)
    # the reference's raw calls have the structure the catalogue test demands of the restatement
    for s in GOLD[f"raw_{i}"]:
        u = s / np.array([[h - P], [w - P]], float) * np.array([[Hg], [Wg]], float)
        cell = np.floor(u).astype(np.int64)
        assert len({tuple(c) for c in cell.T.tolist()}) == n and (cell >= 0).all() and (cell[0] < Hg).all() and (cell[1] < Wg).all()
        assert ((u - cell) >= 0.1 - 1e-9).all() and ((u - cell) <= 0.9 + 1e-9).all()
        check_samples_host_varlen(s.T.astype(np.int64), None, [(h, w)], [n], 1, P)
    # random ORDER, as np.random.choice gives: the first sample's cell is not always the same one
    first = {tuple(SM.segment(SEED, key, 0, n, Hg, Wg, h - P, w - P, 13107).cells[0]) for key in range(40)}
    assert len(first) > 1


def test_plan_samples_reproduces_the_reference_table():
    tab, levels, counts = GOLD["table"], GOLD["table_levels"], GOLD["table_counts"]
    assert len(tab) > 300
    seen_short = seen_zero = False
    for (h, w, count, ns, ratio, P), L, per in zip(tab.tolist(), levels.tolist(), counts.tolist()):
        h, w, count, ns, P = int(h), int(w), int(count), int(ns), int(P)
        assert sampling.compute_patch_num_scales(ns, h, w, P, P) == L == SM.level_count(ns, h, w, P)
        assert sampling.compute_num_patches_per_scale(count, L, ratio).tolist() == per[:L]
        assert SM.level_patches(count, L, ratio).tolist() == per[:L][::-1]
        seen_short, seen_zero = seen_short or L < ns, seen_zero or 0 in per[:L]
        plan = sampling.plan_samples([(h, w)], count, ns, ratio, P)
        want = [(s, per[L - 1 - s]) for s in range(L) if per[L - 1 - s] > 0]              # level s gets the reference's entry -1 - s
        assert [(r[6], r[1]) for r in plan.seg.tolist()] == want and plan.levels == [L] and plan.total == count == sum(per)
        for first, n, Hg, Wg, hm, wm, s, spare in plan.seg.tolist():
            assert (Hg, Wg) == SM.grid(n, h >> s, w >> s) and (hm, wm) == ((h >> s) - P, (w >> s) - P) and spare == 0 and hm >= 0 and wm >= 0
        assert plan.seg[:, 0].tolist() == np.concatenate([[0], np.cumsum(plan.seg[:, 1])[:-1]]).tolist()
    assert seen_short and seen_zero


def test_plan_of_a_batch_is_the_catalogue_tables_back_to_back():
    cases = [c for c in SM.CATALOGUE if c.num_scales == 3 and c.ratio == 1.7 and c.P == 16]
    sizes, counts = [c.size for c in cases], [c.count for c in cases]
    plan = sampling.plan_samples(sizes, counts, 3)
    want = SM.table(sizes, counts, 3, 1.7, 16)
    assert plan.seg.dtype == np.int32 and plan.seg.shape == (len(want), 8) and plan.seg_image.tolist() == [t[0] for t in want]
    assert [tuple(r[:7]) for r in plan.seg.tolist()] == [t[1:] for t in want]
    assert plan.lengths.tolist() == counts and plan.levels == [1, 2, 3, 3, 3]
    assert sampling.plan_samples(sizes[:1], counts[0], 3).seg.tolist() == plan.seg[:1].tolist()


def test_python_layer_refuses_what_is_not_built_by_name():
    s = sampling.PatchSampler()
    assert s.amount_q == 13107 == SM.amount_q(0.2) and sampling.PatchSampler(perturbed_amount=0.5).amount_q == 32768
    assert sampling.PatchSampler(perturbed_amount=0.0, uniform_weight=2.0, diff_type=sampling.DIFF_TYPE_DARK).amount_q == 0
    for kw, word in ((dict(grid_type=sampling.GRID_TYPE_PERTURBED), "GRID_TYPE_PERTURBED"), (dict(grid_type=sampling.GRID_TYPE_HALTON), "GRID_TYPE_HALTON"),
                     (dict(diff_weight=0.5), "diff_weight"), (dict(centerbias_weight=0.5), "centerbias_weight")):
        with pytest.raises(NotImplementedError, match=word):
            sampling.PatchSampler(**kw)
    with pytest.raises(ValueError):
        sampling.PatchSampler(uniform_weight=0.0)
    with pytest.raises(ValueError):
        sampling.PatchSampler(perturbed_amount=1.0)
    with pytest.raises(NotImplementedError, match="randomize_patch_scale_order"):
        sampling.sample_patches([(64, 64)], 10, [0], randomize_patch_scale_order=True)
    with pytest.raises(ValueError, match="8192"):
        sampling.plan_samples([SM.OVER_LIMIT.size], SM.OVER_LIMIT.count)
    with pytest.raises(ValueError, match="smaller than one"):
        sampling.plan_samples([(15, 64)], 4)
    with pytest.raises(ValueError, match="num_scales"):
        sampling.plan_samples([(160, 200)], 2, 3)
    with pytest.raises(ValueError):
        sampling.plan_samples([(160, 200)], [4, 4], 1)
    assert sampling.repeat_key(7, 0) == 7 and sampling.repeat_key(-1, 0) == 2 ** 64 - 1
    assert len({sampling.repeat_key(7, r) for r in range(4)} | {sampling.repeat_key(8, r) for r in range(4)}) == 8
    assert sampling.repeat_key(0, 1) == 0xe220a8397b1dcdaf               # splitmix64's first output from state 0
    assert sampling.as_keys([1, -1, 2 ** 64 + 3], 3).tolist() == [1, 2 ** 64 - 1, 3]


def test_sampled_batch_plan_counts_repeats_against_pairs_and_patches_not_bytes():
    from vtamiq_amd.pipeline import plan_sampled_batch
    sizes = [(48, 64), (160, 200)]
    nbytes = 2 * 3 * (48 * 64 + 160 * 200)
    cap = dict(max_images=12, max_image_bytes=nbytes, max_patches=180, num_scales=3)
    sb = plan_sampled_batch(sizes, sizes, [30, 30], [30, 30], [5, 6], [5, 6], repeats=3, **cap)
    b, t = sb.batch, sb.batch.tables
    assert len(b.sizes) == 12 and b.n_first == 6 and sb.n_images == 4 and sb.repeats == 3 and t.total == 360 and t.image_bytes == nbytes
    assert b.sizes == (sizes * 3) * 2 and b.lengths.tolist() == [30] * 12
    # table rows of repeat r point at the bytes of repeat 0; every row owns its own patch rows
    off = t.img_off.tolist()
    assert off[:6] == off[:2] * 3 and off[6:] == off[6:8] * 3 and off[0] == 0 and off[6] == 3 * (48 * 64 + 160 * 200)
    assert t.row0.tolist() == list(range(0, 361, 30)) and (t.patch_img == np.repeat(np.arange(12), 30)).all()
    assert (t.tab[:, 2:] == np.array(b.sizes)).all() and t.tab.flags["C_CONTIGUOUS"]
    # keys: repeat 0 the pair's own, later repeats derived; both images of a pair the same
    want = [sampling.repeat_key(k, r) for r in range(3) for k in (5, 6)] * 2
    assert sb.seg_keys.tolist() == [want[i] for i in sampling.plan_samples(b.sizes, 30, 3).seg_image.tolist()]
    assert sb.seg.shape[1] == 8 and sb.seg[:, 1].sum() == 360 and sb.seg_at % 4 == 0 and sb.seg_at >= 4 * 12 + 360
    assert sb.front == sb.seg_at + 10 * len(sb.seg) and b.words == sb.front + 3 * 360
    assert b.words <= 4 * 12 + 2 * 180 * 4 + 10 * 3 * 12 + 4, "the slot block of a pipeline with these capacities holds the batch"
    with pytest.raises(ValueError, match="repeats"):
        plan_sampled_batch(sizes, sizes, [30, 30], [30, 30], [5, 6], [5, 6], repeats=4, **cap)                       # 16 table rows of 12
    with pytest.raises(ValueError, match="repeats"):
        plan_sampled_batch(sizes, sizes, [31, 30], [31, 30], [5, 6], [5, 6], repeats=3, **cap)                       # 183 patches a side
    with pytest.raises(ValueError, match="max_image_bytes"):
        plan_sampled_batch(sizes, sizes, [30, 30], [30, 30], [5, 6], [5, 6], repeats=1, **dict(cap, max_image_bytes=nbytes - 1))
    with pytest.raises(ValueError):
        plan_sampled_batch(sizes, sizes, [30, 30], [30, 30], [5], [5, 6], **cap)
    one = plan_sampled_batch(sizes, sizes[::-1], [30, 30], [30, 30], [5, 6], [7, 8], **cap)
    assert one.batch.tables.img_off.tolist() == np.concatenate([[0], np.cumsum([3 * h * w for h, w in sizes + sizes[::-1]])[:-1]]).tolist()


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------------
def test_sampler_header_declares_exactly_the_bound_entry_and_the_library_exports_it():
    header = open(os.path.join(ROOT, "include", "vtamiq_hip_sampler.h")).read()
    declared = set(re.findall(r"\b(vtq_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SAMPLER_SIGNATURES) == {"vtq_k_sample_grid"}
    for other in ("vtamiq_hip.h", "vtamiq_hip_images.h", "vtamiq_hip_rollout.h", "vtamiq_hip_fp8.h"):
        assert "vtq_k_sample_grid" not in open(os.path.join(ROOT, "include", other)).read()
    assert not set(_lib.SAMPLER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.ROLLOUT_SIGNATURES) | set(_lib.IMAGE_SIGNATURES) | set(_lib.FP8_SIGNATURES))
    lib = _lib.load()
    assert hasattr(lib, "vtq_k_sample_grid") and lib.vtq_abi_version() == _lib.ABI_VERSION == 10
    args = [a.strip() for a in re.search(r"vtq_k_sample_grid\((.*?)\);", header, re.S).group(1).split(",")]
    ctype = {"const int32_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)), "const uint64_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)),
             "int32_t*": (ctypes.c_void_p,), "void*": (ctypes.c_void_p,), "int32_t": (ctypes.c_int32,), "uint64_t": (ctypes.c_uint64,)}
    bound = _lib.SAMPLER_SIGNATURES["vtq_k_sample_grid"][1]
    assert len(args) == len(bound) == 10
    for a, b in zip(args, bound):
        assert b in ctype[a.rsplit(" ", 1)[0]], (a, b)
    assert [a.rsplit(" ", 1)[1] for a in args] == ["seg", "keys", "seg_host", "keys_host", "NS", "seed", "amount_q", "samples", "scale_ids", "stream"]
    assert int(re.search(r"#define VTQ_SAMPLER_MAX_CELLS (\d+)", header).group(1)) == sampling.MAX_CELLS == SM.MAX_CELLS == 8192
    from vtamiq_amd import build
    assert "patch_sampler.hip" in build.SOURCES and any(d.endswith("vtamiq_hip_sampler.h") for d in build.DEPS)
    assert "patch_sampler.hip" in open(os.path.join(build.CSRC, "kernels.h")).read()


def test_entry_refuses_bad_arguments_without_a_device():
    """Every refusal of include/vtamiq_hip_sampler.h is decided on HOST arrays before any HIP call: they can be provoked here, with made-up
    device addresses that are never dereferenced."""
    lib = _lib.load()
    plan = sampling.plan_samples([(160, 200), (64, 64)], 30, 3)
    keys = np.arange(len(plan.seg), dtype=np.uint64)
    DEV = 0x10000

    def call(**kw):
        a = dict(seg=DEV, keys=DEV, seg_host=plan.seg, keys_host=keys, NS=len(plan.seg), seed=1, q=13107, samples=DEV, scale_ids=DEV)
        a.update(kw)
        sh = a["seg_host"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a["seg_host"] is not None else None
        kh = a["keys_host"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if a["keys_host"] is not None else None
        rc = lib.vtq_k_sample_grid(a["seg"], a["keys"], sh, kh, a["NS"], a["seed"], a["q"], a["samples"], a["scale_ids"], None)
        return rc, lib.vtq_last_error().decode()

    def edit(row, col, value):
        t = plan.seg.copy()
        t[row, col] = value
        return dict(seg_host=t)

    over = np.array([[0, 8193, 65, 129, 48, 112, 0, 0]], np.int32)        # SM.OVER_LIMIT as a raw table
    assert [tuple(over[0, 1:4])] == [e[1:] for e in SM.OVER_LIMIT.expect]
    cases = {k: {k: None} for k in ("seg", "keys", "seg_host", "keys_host", "samples")}
    cases.update({
        "NS < 1": dict(NS=0), "seg unaligned": dict(seg=DEV + 8), "n < 1": edit(1, 1, 0), "n > Hg Wg": edit(0, 1, 21),
        "more than 8192 cells": dict(seg_host=over, NS=1), "8192 x 2 cells": dict(seg_host=np.array([[0, 5, 8192, 2, 1, 1, 0, 0]], np.int32), NS=1),
        "Hg = 0": edit(0, 2, 0), "negative h - P": edit(0, 4, -1), "negative w - P": edit(2, 5, -1), "w - P of 2^26": edit(0, 5, 1 << 26),
        "level 4": edit(2, 6, 4), "level -1": edit(0, 6, -1), "first row not the prefix": edit(1, 0, 19), "first row of segment 0": edit(0, 0, 1),
        "scale_ids NULL with levels": dict(scale_ids=None), "amount_q -1": dict(q=-1), "amount_q 65536": dict(q=65536)})
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_sample_grid:"), (name, rc, msg)
    assert "8192" in call(**cases["more than 8192 cells"])[1], "the refusal names the limit"
