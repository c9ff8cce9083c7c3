"""The weighted device sampler's definition (include/vtamiq_hip_weighted_sampler.h) as restated in tests/weighted_sampler_model.py, held to
the reference's recorded behaviour (tests/golden/weighted_sampler_reference.npz, written by tests/golden/make_weighted_sampler_golden.py from
the reference's PatchSampler(grid_type=GRID_TYPE_PERTURBED, diff_weight, uniform_weight)), and the host side of vtamiq_amd.sampling's
weighted entries.  No GPU: tests/test_gpu_weighted_sampler.py demands the kernels' bits equal the restatement."""
import os

import numpy as np
import pytest

from tests import weighted_sampler_model as WM
from vtamiq_amd import _lib, sampling

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_sampler_reference.npz")
SEED = 2016
Q = 13107
KEYS = 4000


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def _distance(a, b, n):
    """L1 distance of two per-cell mean occupancies, in units of the n samples of a call."""
    return float(np.abs(a - b).sum()) / n


def _check_draw(seg, h, w, n, cs, sh, sw, P):
    """One draw of the restatement: exactly n samples, each inside the level and inside the extent of the cell it was drawn for."""
    s = seg.samples.astype(np.int64)
    assert s.shape == (n, 2) and seg.k.sum() == n
    assert (s >= 0).all() and (s[:, 0] <= h - P).all() and (s[:, 1] <= w - P).all()
    j, i = seg.cell // sw, seg.cell % sw
    er, ec = WM.extents(h - P, cs, sh), WM.extents(w - P, cs, sw)
    assert ((s[:, 0] >= j * cs) & (s[:, 0] <= j * cs + er[j]) & (s[:, 1] >= i * cs) & (s[:, 1] <= i * cs + ec[i])).all()
    assert np.array_equal(np.bincount(seg.cell, minlength=sh * sw), seg.k)


def _mean_occupancy(h, w, n, cs, sh, sw, P, dw, uw, tab, keys):
    """Per-cell mean occupancy over `keys`; every draw is held to _check_draw on the way."""
    occ = np.zeros(sh * sw)
    for key in keys:
        seg = WM.segment(SEED, key, 0, n, cs, sh, sw, h - P, w - P, P, Q, dw, uw, tab, 0 if tab is not None else -1, 4 if tab is not None else -1)
        _check_draw(seg, h, w, n, cs, sh, sw, P)
        occ += WM.occupancy(seg.samples, cs, sh, sw)
    return occ / len(keys)


# ---- 1: allocation, against the reference's records -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("weighting", [0, 1])
def test_allocation_is_as_close_to_the_reference_as_the_reference_is_to_itself(ref, shape, weighting):
    """D(restatement over 4000 keys, record A) <= 1.5 D(A, B), A and B two independent records of K = 400 reference calls on the hot-spot
    map; with the difference term dropped the restatement misses that gate at least tenfold (200 keys suffice to see it).  Every one of
    the draws also has exactly n samples inside the level and inside their cells (_check_draw)."""
    h, w, n = ref["shapes"][shape].tolist()
    dw, uw = ref["weights"][weighting].tolist()
    cs, sh, sw = ref[f"cells_{shape}"].tolist()
    P, K = int(ref["P"]), int(ref["K"])
    assert (cs, sh, sw) == WM.geometry(n, h, w, P) == sampling.cell_geometry(n, h, w, P)
    A, B = ref[f"occupancy_A_{shape}_{weighting}"] / K, ref[f"occupancy_B_{shape}_{weighting}"] / K
    assert A.sum() == pytest.approx(n) and B.sum() == pytest.approx(n)
    F = _distance(A, B, n)
    tab = WM.map_table(WM.hot_spot_map(h, w), cs, sh, sw, P)
    D = _distance(_mean_occupancy(h, w, n, cs, sh, sw, P, dw, uw, tab, range(KEYS)), A, n)
    D0 = _distance(_mean_occupancy(h, w, n, cs, sh, sw, P, 0.0, 1.0, None, range(200)), A, n)
    print(f"{h}x{w} / {n}, dw {dw}, uw {uw}: F = {F:.5f}, D = {D:.5f} = {D / F:.2f} F, without the difference term {D0 / F:.1f} F")
    assert D <= 1.5 * F
    assert D0 >= 10 * 1.5 * F


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
@pytest.mark.parametrize("weighting", [0, 1])
def test_every_call_has_n_samples_inside_the_level_and_inside_their_cells(ref, shape, weighting):
    """The raw reference calls and the restatement's draws: exactly n samples, each inside [0, h - P] x [0, w - P]; the restatement's also
    inside the extent of the cell they were drawn for (the jitter is clipped to the cell).  64 x 80 / 24, where the ceilings dominate
    the allocation, is held to this and its occupancy distance is printed, not gated."""
    h, w, n = ref["shapes"][shape].tolist()
    dw, uw = ref["weights"][weighting].tolist()
    cs, sh, sw = ref[f"cells_{shape}"].tolist()
    P, K = int(ref["P"]), int(ref["K"])
    raw = ref[f"raw_{shape}_{weighting}"]
    assert raw.shape == (8, 2, n)
    assert (raw >= 0).all() and (raw[:, 0] <= h - P).all() and (raw[:, 1] <= w - P).all()
    tab = WM.map_table(WM.hot_spot_map(h, w), cs, sh, sw, P)
    occ = np.zeros(sh * sw)
    for key in range(40):
        seg = WM.segment(SEED, key, 0, n, cs, sh, sw, h - P, w - P, P, Q, dw, uw, tab, 0, 4)
        assert seg.use
        _check_draw(seg, h, w, n, cs, sh, sw, P)
        E = int(seg.k_ceil.sum()) - n
        assert 0 <= E < np.count_nonzero(seg.k_ceil) and ((seg.k_ceil - seg.k) >= 0).all() and (seg.k_ceil - seg.k).max() <= 1
        occ += WM.occupancy(seg.samples, cs, sh, sw)
    A, B = ref[f"occupancy_A_{shape}_{weighting}"] / K, ref[f"occupancy_B_{shape}_{weighting}"] / K
    print(f"{h}x{w} / {n}, dw {dw}, uw {uw}: 40 keys, D = {_distance(occ / 40, A, n):.4f}, F = {_distance(A, B, n):.4f}")


# ---- 2: weights, against compute_diff ------------------------------------------------------------------------------------------------------
WEIGHT_GATE = 2 * 1.975e-3


def test_cell_weights_are_the_references_cell_probabilities(ref):
    """S_c / sum of S_c of the restatement against the cell probabilities the reference derives through compute_diff (uniform_weight = 0)
    from the three uint8 pairs of the fixture, level by level.  The only modelled loss is the isqrt floor, under one unit of Ra Rb per
    pixel.  Measured worst relative difference: 1.975e-3 (pair 2 = 71 x 85, level 0, a cell holding 0.27 % of the weight; the other levels
    5.4e-4 and below); the gate is twice that.  A cell without weight in the reference has none here."""
    P, worst = int(ref["P"]), 0.0
    for p in range(3):
        a, b = ref[f"pair_{p}_a"], ref[f"pair_{p}_b"]
        m0, (amin, amax, bmin, bmax) = WM.pixel_weight(a, b)
        assert amax - amin >= 200 and bmax - bmin >= 200
        for level, n in enumerate(ref[f"pair_{p}_counts"].tolist()):
            m = WM.pool(m0, level)
            cs, sh, sw = ref[f"pair_{p}_cells_{level}"].tolist()
            assert m.shape == (a.shape[0] >> level, a.shape[1] >> level) and (cs, sh, sw) == WM.geometry(n, *m.shape, P)
            S = WM.cell_sums(m, cs, sh, sw, P).astype(np.float64)
            want = ref[f"pair_{p}_prob_{level}"].reshape(-1)
            got = S / S.sum()
            assert np.array_equal(got == 0, want == 0)
            rel = np.abs(got - want)[want > 0] / want[want > 0]
            print(f"pair {p} level {level}: {m.shape}, cells {sh} x {sw} of {cs}: worst relative difference {rel.max():.3e}")
            worst = max(worst, float(rel.max()))
    assert worst <= WEIGHT_GATE
    ranges = [(int(ref[f"pair_{p}_a"].max()) - int(ref[f"pair_{p}_a"].min()), int(ref[f"pair_{p}_b"].max()) - int(ref[f"pair_{p}_b"].min())) for p in range(3)]
    assert any(ra != rb for ra, rb in ranges) and ref["pair_2_a"].shape[0] % 2 == 1 and len(ref["pair_2_counts"]) == 3


# ---- 3: the restatement itself ---------------------------------------------------------------------------------------------------------------
def test_a_segment_is_a_pure_function_of_its_arguments():
    h, w, n, P = 96, 128, 60, 16
    cs, sh, sw = WM.geometry(n, h, w, P)
    tab = WM.map_table(WM.hot_spot_map(h, w), cs, sh, sw, P)
    base = dict(seed=SEED, key=5, level=0, n=n, cs=cs, sh=sh, sw=sw, hm=h - P, wm=w - P, P=P, q=Q, dw=1.0, uw=0.1, tab=tab, head=0, off=4)
    one = WM.segment(**base).samples
    assert np.array_equal(one, WM.segment(**base).samples)
    moved = np.concatenate([np.full(7, 2 ** 64 - 1, np.uint64), tab, np.full(5, 2 ** 64 - 1, np.uint64)])     # the same words elsewhere, other words around
    assert np.array_equal(one, WM.segment(**dict(base, tab=moved, head=7, off=11)).samples)
    other = tab.copy()
    other[4 + 2 + 3] += np.uint64(50000)
    for change in (dict(seed=SEED + 1), dict(key=6), dict(level=1), dict(q=2 * Q), dict(uw=0.2), dict(dw=2.0), dict(tab=other), dict(n=n + 1)):
        assert not np.array_equal(one, WM.segment(**dict(base, **change)).samples[:n]), change


def test_without_a_difference_term_the_counts_follow_the_window_areas():
    for (h, w, n, P) in ((96, 128, 60, 16), (64, 80, 24, 16), (45, 77, 30, 8)):
        cs, sh, sw = WM.geometry(n, h, w, P)
        A = WM.window_areas(h, w, cs, sh, sw, P)
        want = np.ceil(n * A.astype(np.float64) / A.sum()).astype(np.int64)
        tab = WM.map_table(WM.hot_spot_map(h, w), cs, sh, sw, P)
        for kw in (dict(dw=0.0, uw=1.0), dict(dw=0.0, uw=0.3, tab=tab, head=0, off=4), dict(dw=1.0, uw=1.0),                   # no table
                   dict(dw=1.0, uw=1.0, tab=WM.map_table(np.full((h, w), 9), cs, sh, sw, P), head=0, off=4),                    # variance 0
                   dict(dw=1.0, uw=1.0, tab=WM.map_table(WM.hot_spot_map(h, w), cs, sh, sw, P, Ra=0), head=0, off=4)):         # a constant image
            seg = WM.segment(SEED, 1, 0, n, cs, sh, sw, h - P, w - P, P, Q, **kw)
            assert not seg.use and np.array_equal(seg.k_ceil, want), kw


# ---- 4: the host side of vtamiq_amd.sampling ----------------------------------------------------------------------------------------------
def test_the_plan_is_the_restatements_table():
    sizes, counts = [(160, 200), (16, 64), (301, 403), (80, 80), (17, 40)], [30, 4, 100, 31, 5]
    for ns, P in ((1, 16), (3, 16), (4, 16), (3, 8)):
        plan = sampling.plan_samples_weighted(sizes, counts, ns, 1.7, P)
        rows = WM.table(sizes, counts, ns, 1.7, P)
        assert plan.seg.shape == (len(rows), 12) and plan.seg.dtype == np.int32 and plan.total == sum(counts)
        assert [tuple(r[:8]) for r in plan.seg.tolist()] == [r[1:] for r in rows] and plan.seg_image.tolist() == [r[0] for r in rows]
        assert plan.lev.shape[0] == len(rows) and plan.pairs.shape == (len(sizes), 8)
        T = 0
        for p in range(len(sizes)):
            mine = [r for r in plan.lev.tolist() if r[0] == p]
            assert plan.pairs[p].tolist()[2:] == [sizes[p][0], sizes[p][1], T, plan.lev[:, 0].tolist().index(p), len(mine), 0]
            head, T = T, T + 4
            for r in mine:
                assert r[5:7] == [head, T]
                T += 2 + r[3] * r[4]
        assert T == plan.tab_words
        assert np.array_equal(plan.seg[:, 8:10], plan.lev[:, 5:7])
    both = sampling.plan_samples_weighted(sizes * 2, counts * 2, 3, pair_of=list(range(5)) * 2)
    one = sampling.plan_samples_weighted(sizes, counts, 3)
    assert np.array_equal(both.lev, one.lev) and np.array_equal(both.pairs, one.pairs) and both.tab_words == one.tab_words
    assert np.array_equal(both.seg[len(one.seg):, 1:], one.seg[:, 1:]) and np.array_equal(both.seg[:len(one.seg)], one.seg)


def test_every_refusal_fires_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_library)
    W = sampling.WeightedPatchSampler
    with pytest.raises(NotImplementedError, match="centerbias_weight"):
        W(1.0, 0.1, centerbias_weight=0.5)
    with pytest.raises(NotImplementedError, match="DIFF_TYPE_DARK"):
        W(1.0, 0.1, diff_type=sampling.DIFF_TYPE_DARK)
    with pytest.raises(ValueError, match="Total weight must be non-zero"):
        W(0.0, 0.0)
    with pytest.raises(ValueError, match="Total weight must be non-zero"):
        W(-1.0, 1e-7)
    with pytest.raises(ValueError, match="perturbed_amount"):
        W(1.0, 0.1, perturbed_amount=1.5)
    s = W(1.0, 0.1)
    assert (s.diff_weight, s.uniform_weight, s.amount_q, s.grid_type) == (1.0, 0.1, Q, sampling.GRID_TYPE_PERTURBED)
    assert W(0.0, 1.0, diff_type=sampling.DIFF_TYPE_DARK).diff_weight == 0.0        # the reference never looks at diff_type then
    plan = sampling.plan_samples_weighted
    for bad, match in ((dict(sizes=[(15, 64)], patch_count=4), "smaller than one"), (dict(sizes=[(64, 64)], patch_count=2, num_scales=3), "below num_scales"),
                       (dict(sizes=[(2048, 2049)], patch_count=100), "2\\^22"), (dict(sizes=[(64, 64)], patch_count=8101), "8100"),
                       (dict(sizes=[(64, 64)], patch_count=4, patch_size=4), "patch_size"), (dict(sizes=[(64, 64)], patch_count=4, num_scales=5), "num_scales"),
                       (dict(sizes=[(64, 64), (64, 80)], patch_count=4, pair_of=[0, 0]), "one table"),
                       (dict(sizes=[(64, 64), (64, 64)], patch_count=[4, 5], pair_of=[0, 0]), "one table"),
                       (dict(sizes=[(64, 64), (64, 64)], patch_count=4, pair_of=[0, 2]), "pair_of"), (dict(sizes=[], patch_count=4), "sizes")):
        with pytest.raises(ValueError, match=match):
            plan(**bad)
    with pytest.raises(TypeError, match="WeightedPatchSampler"):
        sampling.sample_patches_weighted(None, [0, 0], [(64, 64)], 4, [1], sampling.PatchSampler())
    with pytest.raises(RuntimeError, match="GPU"):
        sampling.sample_patches_weighted(np.zeros(10, np.uint8), [0, 0], [(64, 64)], 4, [1], s)


def test_the_default_samplers_refusals_are_unchanged():
    S = sampling.PatchSampler
    with pytest.raises(NotImplementedError, match="GRID_TYPE_PERTURBED is not built"):
        S(grid_type=sampling.GRID_TYPE_PERTURBED)
    with pytest.raises(NotImplementedError, match="GRID_TYPE_HALTON is not built"):
        S(grid_type=sampling.GRID_TYPE_HALTON)
    with pytest.raises(NotImplementedError, match="diff_weight > 0 is not built"):
        S(diff_weight=1.0)
    with pytest.raises(NotImplementedError, match="centerbias_weight > 0 is not built"):
        S(centerbias_weight=1.0)
    with pytest.raises(ValueError, match="Total weight must be non-zero"):
        S(uniform_weight=0.0)
    assert S().amount_q == Q and not isinstance(S(), sampling.WeightedPatchSampler)
