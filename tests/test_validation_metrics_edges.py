"""The validation reductions where a validation set degenerates: constant scores (a collapsed model), NaN, +-inf, ranges around the 1e-6
no-divide branch of normalize_array, +-0.0, exact monotone orders, n = 5, pair counts beyond 2^32.

tests/golden/validation_metrics_edges.npz holds what the reference's own compute_correlations_cat_flat / compute_correlations /
average_over_repeats return for 17 such inputs (tests/golden/make_golden.py:run_validation_metrics_edges), NaN and inf as they come.
CPU: oracle/metrics_oracle.py reproduces every stored field, and the host half of vtamiq_amd.validate (tau-b from the pair counts, the fit,
PLCC / RMSE) does so from the oracle's normalised vectors.  GPU: the HIP kernels through the Python entries and through vtq_k_rank_metrics /
vtq_k_repeat_mean directly.

A field compares as: NaN matches NaN, an infinity matches by equality, a finite value within TOL of tests/test_validation_metrics.py.
"""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO
from tests.test_validation_metrics import FIELDS, TOL

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "validation_metrics_edges.npz"))
CASES = ["const_pred", "const_target", "const_both", "all_but_one_equal", "range_below_eps", "range_above_eps", "nan_first", "nan_last",
         "nan_in_target", "nan_one_repeat", "neg_inf", "pos_inf", "all_nan", "monotone", "antitone", "signed_zero", "n5"]
NONORM_CASES = ["pos_inf", "nan_first"]                    # also stored for compute_correlations(a, b, normalize=False)
FP64_CASES = {"range_below_eps", "range_above_eps"}        # fp32 cannot hold 1 + 5e-7: these enter compute_correlations as fp64 vectors
NOFIT = ["SROCC", "KROCC", "PLCC_NOFIT", "RMSE_NOFIT"]


def same(got, want, field):
    got, want = float(got), float(want)
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= TOL[field]


def check_fields(got, want, fields=FIELDS, what=""):
    bad = {f: (float(got[f]), float(want[f])) for f in fields if not same(got[f], want[f], f)}
    assert not bad, (what, bad)


def stored(name, nonorm=False):
    assert list(G["field_names"]) == FIELDS
    return dict(zip(FIELDS, G[name + ("_nonorm_fields" if nonorm else "_fields")]))


def batches(name):
    """The per-batch lists the validation loop would hand to compute_correlations_cat_flat: `reps` passes over the set in batches of `bs`."""
    q, pred, reps, bs = G[name + "_q"], G[name + "_pred"], int(G[name + "_reps"]), int(G[name + "_bs"])
    n = q.size
    ys = [q[i:i + bs] for _ in range(reps) for i in range(0, n, bs)]
    yp = [pred[r * n + i:r * n + min(i + bs, n)] for r in range(reps) for i in range(0, n, bs)]
    return ys, yp, reps


def vectors(name):
    """The two fp64 vectors that enter compute_correlations for a case (after the cat and the mean over repeats)."""
    ys, yp, reps = batches(name)
    a, b = (np.concatenate([np.asarray(t, dtype=float).ravel() for t in l]) for l in (ys, yp))
    if reps > 1:
        a, b = MO.average_over_repeats(a, reps), MO.average_over_repeats(b, reps)
    return a, b


def quiet(fn, *args, **kw):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def bits_equal(x, y):
    """Bit for bit, except that any NaN matches any NaN."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x.view(np.int64)[~nx], y.view(np.int64)[~ny])


# ---- CPU: the fixture says what the issue's table says, and the oracle reproduces it ------------------------------------------------------
def test_fixture_holds_the_degenerate_answers():
    """The stored reference results are the degenerate ones: were they all finite, every comparison below would be an ordinary parity check."""
    assert sorted(k[:-len("_fields")] for k in G.files if k.endswith("_fields") and "_nonorm" not in k) == sorted(CASES)
    for name in ("const_pred", "const_target", "const_both"):
        s = stored(name)
        assert all(math.isnan(s[f]) for f in ("SROCC", "KROCC", "PLCC_NOFIT", "PLCC")) and all(math.isfinite(s[f]) for f in ("RMSE", "RMSE_NOFIT"))
    for name in ("nan_first", "nan_last", "nan_in_target", "nan_one_repeat", "neg_inf", "pos_inf", "all_nan"):
        assert all(math.isnan(v) for v in stored(name).values()), name
    assert all(math.isnan(v) for v in stored("nan_first", nonorm=True).values())
    s = stored("pos_inf", nonorm=True)
    assert math.isfinite(s["SROCC"]) and math.isfinite(s["KROCC"]) and math.isnan(s["PLCC_NOFIT"]) and math.isnan(s["PLCC"])
    assert s["RMSE_NOFIT"] == math.inf and s["RMSE"] == math.inf
    for name in ("all_but_one_equal", "range_below_eps", "range_above_eps", "monotone", "antitone", "signed_zero", "n5"):
        assert all(math.isfinite(v) for v in stored(name).values()), name
    assert abs(stored("monotone")["SROCC"] - 1) < 1e-12 and abs(stored("monotone")["KROCC"] - 1) < 1e-12
    assert abs(stored("antitone")["SROCC"] + 1) < 1e-12 and abs(stored("antitone")["KROCC"] + 1) < 1e-12
    for name in FP64_CASES:
        assert G[name + "_pred"].dtype == np.float64 and 0 < np.ptp(G[name + "_pred"]) < 1e-5
    assert np.ptp(G["range_below_eps_pred"]) < 1e-6 < np.ptp(G["range_above_eps_pred"])
    z = G["signed_zero_pred"]
    assert (z[z == 0].size >= 2 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and (z < 0).any() and (z > 0).any())
    assert G["n5_q"].size == 5 and int(G["nan_one_repeat_reps"]) == 3
    p = G["nan_one_repeat_pred"].reshape(3, -1)
    assert np.isnan(p).sum() == 1 and np.isnan(G["nan_one_repeat_mean"]).sum() == 1


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_edges(name):
    ys, yp, reps = batches(name)
    if name in FP64_CASES:
        got = quiet(MO.compute_correlations, G[name + "_q"], G[name + "_pred"])
    else:
        got = quiet(MO.compute_correlations_cat_flat, ys, yp, reps)
    check_fields(got, stored(name), what=name)
    if reps > 1:
        assert bits_equal(MO.average_over_repeats(G[name + "_pred"], reps), G[name + "_mean"])


@pytest.mark.parametrize("name", NONORM_CASES)
def test_oracle_reproduces_reference_edges_unnormalised(name):
    a, b = vectors(name)
    check_fields(quiet(MO.compute_correlations, a, b, normalize=False), stored(name, nonorm=True), what=name)


def _pair_counts(aa, bb):
    """What pair_kernel counts, in numpy: sums over ORDERED pairs, a NaN comparing as tied with everything."""
    da = (aa[:, None] > aa[None, :]).astype(int) - (aa[:, None] < aa[None, :])
    db = (bb[:, None] > bb[None, :]).astype(int) - (bb[:, None] < bb[None, :])
    n = aa.size
    return float((da * db).sum()), float((da == 0).sum() - n), float((db == 0).sum() - n)


@pytest.mark.parametrize("name", CASES + [n + "/nonorm" for n in NONORM_CASES])
def test_host_half_reproduces_reference_edges(name):
    """vtamiq_amd.validate._finish_correlations (tau-b from the counts, the fit, PLCC / RMSE) fed what the device is required to hand it --
    numpy's normalised vectors, the exact counts, scipy's fit-free statistics -- returns the reference's six fields.  The three const_* cases
    included at the full tolerance: their fitted fields are NaN (PLCC) and an RMSE that MINPACK reproduces to 1e-10, against TOL["RMSE"] = 1e-6."""
    import scipy.stats
    from vtamiq_amd import validate
    name, _, nonorm = name.partition("/")
    a, b = vectors(name)
    aa, bb = (a.copy(), b.copy()) if nonorm else (quiet(MO.normalize_array, a), quiet(MO.normalize_array, b))
    fitfree = [quiet(lambda: scipy.stats.spearmanr(aa, bb).correlation), quiet(lambda: scipy.stats.pearsonr(aa, bb)[0]),
               quiet(lambda: float(np.sqrt(np.mean((aa - bb) ** 2))))]
    host = np.concatenate([fitfree, _pair_counts(aa, bb), aa, bb])
    check_fields(quiet(validate._finish_correlations, host, a.size), stored(name, nonorm=bool(nonorm)), what=name)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


CONST_CASES = {"const_pred", "const_target", "const_both"}


def identical(x, y, fields=FIELDS):
    return all((x[f] == y[f]) or (math.isnan(x[f]) and math.isnan(y[f])) for f in fields)


def same_nanness(x, y, fields=("PLCC", "RMSE")):
    return all(math.isnan(x[f]) == math.isnan(y[f]) for f in fields)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_metrics_match_reference_edges(name):
    """Every fixture case through compute_correlations_cat_flat (the fp64 range cases through compute_correlations: the cat path casts to
    fp32), direct and deferred.  Both results meet all six stored fields at the TOL table, no case relaxed, and the deferred result is the
    direct one bit for bit -- except the two fitted fields of const_pred, const_target and const_both, compared between the two for NaN-ness
    only: with a constant vector the Jacobian of the logistic fit is rank-deficient, and scipy.optimize.leastsq then returns different last
    digits for IDENTICAL inputs and an identical history of residual evaluations (on the CPU alone, 3 000 repeats of const_pred: RMSE
    0.3046117163630402 2 737 times, 0.30461171639773893 -- the stored value -- 261 times, 0.30461171640427387 twice; all 3.5e-11 apart
    against TOL["RMSE"] = 1e-6)."""
    from vtamiq_amd import validate
    ys, yp, reps = batches(name)
    if name in FP64_CASES:
        a, b = dev(G[name + "_q"]), dev(G[name + "_pred"])
        got = quiet(validate.compute_correlations, a, b)
        pend = quiet(validate.compute_correlations_deferred, a, b)
    else:
        dy, dp = [dev(t) for t in ys], [dev(t) for t in yp]
        got = quiet(validate.compute_correlations_cat_flat, dy, dp, reps)
        pend = quiet(validate.compute_correlations_cat_flat, dy, dp, reps, defer=True)
    later = quiet(pend.result)
    print(name, {f: got[f] for f in FIELDS})
    check_fields(got, stored(name), what=name)
    check_fields(later, stored(name), what=name + " deferred")
    assert pend.done()
    if name in CONST_CASES:
        assert identical(later, got, NOFIT) and same_nanness(later, got), (later, got)
    else:
        assert identical(later, got), (later, got)
    if reps > 1:
        assert bits_equal(validate.average_over_repeats(dev(G[name + "_pred"]), reps).cpu().numpy(), G[name + "_mean"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONORM_CASES)
def test_hip_metrics_match_reference_edges_unnormalised(name):
    from vtamiq_amd import validate
    a, b = vectors(name)
    got = quiet(validate.compute_correlations, dev(a), dev(b), normalize=False)
    later = quiet(quiet(validate.compute_correlations_deferred, dev(a), dev(b), normalize=False).result)
    print(name, {f: got[f] for f in FIELDS})
    check_fields(got, stored(name, nonorm=True), what=name)
    assert identical(later, got), (later, got)


def rank_metrics(a, b, normalize):
    """vtq_k_rank_metrics on two fp64 numpy vectors -> (work [4N], counts [3], out [3]) as numpy."""
    from vtamiq_amd import _lib
    n = a.size
    da, db = dev(np.asarray(a, dtype=np.float64)), dev(np.asarray(b, dtype=np.float64))
    work = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().vtq_k_rank_metrics(da.data_ptr(), db.data_ptr(), n, int(normalize), work.data_ptr(), counts.data_ptr(), out.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return work.cpu().numpy(), [int(c) for c in counts.cpu().numpy()], out.cpu().numpy()


def tau_b(counts, n):
    tot = n * (n - 1) // 2
    cd, xt, yt = (c // 2 for c in counts)
    return cd / math.sqrt(tot - xt) / math.sqrt(tot - yt)


def check_direct(a, b, normalize, what):
    """One vtq_k_rank_metrics call against numpy / scipy: normalised copies bit for bit; without a NaN in them exact ranks and counts that
    give scipy's tau-b (or say "constant"); with one, NaN out[0:3] and the NaN in work[0:2N] from which the host reports Kendall as NaN."""
    import scipy.stats
    n = a.size
    aa, bb = (quiet(MO.normalize_array, a), quiet(MO.normalize_array, b)) if normalize else (a, b)
    work, counts, out = rank_metrics(a, b, normalize)
    assert np.array_equal(work[:n], aa, equal_nan=True) and np.array_equal(work[n:2 * n], bb, equal_nan=True), what
    assert bits_equal(work[:n], aa) and bits_equal(work[n:2 * n], bb), what
    want = {"SROCC": quiet(lambda: scipy.stats.spearmanr(aa, bb).correlation), "PLCC_NOFIT": quiet(lambda: scipy.stats.pearsonr(aa, bb)[0]),
            "RMSE_NOFIT": quiet(lambda: float(np.sqrt(np.mean((aa - bb) ** 2))))}
    got = {"SROCC": out[0], "PLCC_NOFIT": out[1], "RMSE_NOFIT": out[2]}
    print(what, got, counts)
    check_fields(got, want, fields=list(want), what=what)
    if np.isnan(aa).any() or np.isnan(bb).any():
        assert math.isnan(out[0]) and math.isnan(out[1]), (what, out)
        assert np.isnan(work[:2 * n]).any(), what                       # validate._finish_correlations: Kendall is NaN when these hold a NaN
        return
    assert np.array_equal(work[2 * n:3 * n], scipy.stats.rankdata(aa)) and np.array_equal(work[3 * n:], scipy.stats.rankdata(bb)), what
    tot = n * (n - 1) // 2
    kendall = quiet(lambda: scipy.stats.kendalltau(aa, bb).correlation)
    if math.isnan(kendall):                                              # a constant vector: every pair tied, the host's "no tau" condition
        assert counts[1] // 2 == tot or counts[2] // 2 == tot, (what, counts)
    else:
        assert abs(tau_b(counts, n) - kendall) <= TOL["KROCC"], (what, tau_b(counts, n), kendall)


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_rank_metrics_entry_on_reference_edges(name, normalize):
    a, b = vectors(name)
    check_direct(a, b, normalize, f"{name} normalize={normalize}")


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("N", [2, 3])
def test_rank_metrics_entry_constant_vector_below_the_fit_size(N, normalize):
    """N = 2, 3: out of the Python entry's reach (MINPACK needs 5 points).  0.1 is chosen because the mean of three of them is not 0.1: only an
    explicit constant-input rule (scipy.stats.pearsonr's) gives NaN there, the centred sums give +-1."""
    const, other = np.full(N, 0.1), np.array([0.5, 2.0, 1.25])[:N]
    for a, b, what in ((const, other, "a"), (other, const, "b"), (const, const + 0.2, "both")):
        work, counts, out = rank_metrics(a, b, normalize)
        print(N, normalize, what, out, counts)
        assert math.isnan(out[0]) and math.isnan(out[1]) and math.isfinite(out[2]), (N, normalize, what, out)
        check_direct(a, b, normalize, f"constant {what} N={N} normalize={normalize}")


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("value", [math.nan, math.inf])
@pytest.mark.parametrize("N", [257, 1025])
def test_one_nonfinite_score_at_block_and_stride_edges(N, value, side):
    """One NaN / +inf at index 0, 255, 256, N - 1 (the block edges of pair_kernel, the stride edges of the 1024-thread reductions), in the
    targets or in the predictions, normalised or not: the kernel entry against numpy / scipy, and the Python entry's fit-free fields (KROCC
    among them) against the oracle; the fitted fields, host work on vectors asserted bit-equal, for NaN-ness and infinity."""
    from vtamiq_amd import validate
    rng = np.random.default_rng(N)
    a0 = rng.uniform(0, 5, N)
    b0 = 0.6 * a0 + rng.standard_normal(N)
    for idx in (0, 255, 256, N - 1):
        a, b = a0.copy(), b0.copy()
        (a if side == "a" else b)[idx] = value
        for normalize in (0, 1):
            what = f"N={N} {value} in {side}[{idx}] normalize={normalize}"
            check_direct(a, b, normalize, what)
            want = quiet(MO.compute_correlations, a, b, normalize=bool(normalize))
            got = quiet(validate.compute_correlations, dev(a), dev(b), normalize=bool(normalize))
            check_fields(got, want, fields=NOFIT, what=what)
            for f in ("PLCC", "RMSE"):
                assert math.isnan(got[f]) == math.isnan(want[f]) and math.isinf(got[f]) == math.isinf(want[f]), (what, f, got[f], want[f])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("R", [1, 2, 7])
def test_repeat_mean_of_nonfinite_scores(R, N):
    """NaN, +inf, -inf, +inf and -inf in one column (their sum is NaN), -0.0 alone in a column: bit-equal (any NaN matching any NaN) to numpy's
    fp64 reduction over axis 0, the sign of a zero included."""
    from vtamiq_amd import validate
    rng = np.random.default_rng(10 * R + N)
    kinds = ["nan", "+inf", "-inf", "-0", "mixed0"] + (["+inf-inf"] if R > 1 else [])

    def poison(q, col, kind):
        r = int(rng.integers(R))
        if kind == "nan":
            q[r, col] = np.nan
        elif kind == "+inf":
            q[r, col] = np.inf
        elif kind == "-inf":
            q[r, col] = -np.inf
        elif kind == "-0":
            q[:, col] = -0.0
        elif kind == "mixed0":
            q[:, col] = 0.0
            q[r, col] = -0.0
        else:
            q[r, col], q[(r + 1) % R, col] = np.inf, -np.inf

    mats = []
    if N == 1:
        for kind in kinds:
            q = rng.standard_normal((R, 1)).astype(np.float32)
            poison(q, 0, kind)
            mats.append(q)
    else:
        q = rng.standard_normal((R, N)).astype(np.float32)
        for kind, cols in zip(kinds, ((0, 100), (1, 255), (2, 256), (3, N - 1), (4, 254), (5, 128))):
            for col in cols:
                poison(q, col, kind)
        mats.append(q)
    for q in mats:
        want = quiet(MO.average_over_repeats, q.reshape(-1), R)
        got = validate.average_over_repeats(dev(q.reshape(-1)), R).cpu().numpy()
        assert bits_equal(got, want), (R, N, q[:, :6], got[:6], want[:6])


def _exact_spearman(a, b):
    """Pearson of the average-tie ranks in integers: doubled ranks are integers, so r = num / sqrt(da * db) with exact num, da, db."""
    import scipy.stats
    ra = [int(v) for v in np.rint(2 * scipy.stats.rankdata(a))]
    rb = [int(v) for v in np.rint(2 * scipy.stats.rankdata(b))]
    n, sa, sb = len(ra), sum(ra), sum(rb)
    num = n * sum(x * y for x, y in zip(ra, rb)) - sa * sb
    da, db = n * sum(x * x for x in ra) - sa * sa, n * sum(y * y for y in rb) - sb * sb
    return num / math.sqrt(da) / math.sqrt(db)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["increasing", "decreasing", "three_values"])
def test_pair_counts_beyond_32_bits(kind):
    """N = 65 600, the first round size with N (N - 1) > 2^32: the concordance sum (strict orders) or both tie sums (three distinct values,
    all but 60 scores equal) pass 2^32.  KROCC / SROCC against scipy; should SROCC of the tied case miss scipy, the arbiter is the exact
    ratio of integers (ranks are half-integers), which both then have to meet -- the tolerance stays TOL["SROCC"]."""
    import scipy.stats
    N = 65600
    assert N * (N - 1) > 2 ** 32 >= (N - 100) * (N - 101)
    rng = np.random.default_rng(65600)
    if kind == "three_values":
        a, b = np.zeros(N), np.zeros(N)
        pa, pb = rng.permutation(N), rng.permutation(N)
        a[pa[:30]], a[pa[30:60]] = 1.0, 2.0
        b[pa[:20]], b[pa[30:45]] = 1.0, 2.0                              # partly the same scores as in a: some concordant pairs
        b[pb[:10]], b[pb[10:25]] = 1.0, 2.0
    else:
        a = np.sort(rng.uniform(0, 5, N))
        assert (np.diff(a) > 0).all()
        b = 0.6 * a + 1.0 if kind == "increasing" else 3.0 - 0.6 * a
        assert (np.diff(b) != 0).all()
        p = rng.permutation(N)
        a, b = a[p], b[p]
    work, counts, out = rank_metrics(a, b, 0)
    print(kind, counts, out)
    if kind == "three_values":
        assert counts[1] > 2 ** 32 and counts[2] > 2 ** 32
    else:
        assert abs(counts[0]) == N * (N - 1) > 2 ** 32 and counts[1] == 0 and counts[2] == 0
    assert np.array_equal(work[2 * N:3 * N], scipy.stats.rankdata(a)) and np.array_equal(work[3 * N:], scipy.stats.rankdata(b))
    assert abs(tau_b(counts, N) - scipy.stats.kendalltau(a, b).correlation) <= TOL["KROCC"]
    by_scipy = scipy.stats.spearmanr(a, b).correlation
    if kind == "three_values" and abs(out[0] - by_scipy) > TOL["SROCC"]:
        exact = _exact_spearman(a, b)
        print("SROCC device / scipy / exact:", out[0], by_scipy, exact)
        assert abs(out[0] - exact) <= TOL["SROCC"] and abs(by_scipy - exact) > abs(out[0] - exact)
    else:
        assert abs(out[0] - by_scipy) <= TOL["SROCC"], (out[0], by_scipy)


@pytest.mark.gpu
def test_collapsed_model_reports_no_correlation():
    """The small model of test_predict_repeats_equals_separate_passes with the weight of the head's last linear layer zeroed: every score is
    that layer's bias.  The validation pass must say "no correlation" (NaN), not a perfect one; the RMSE fields stay finite.  Deferred against
    direct: bit-identical, the fitted RMSE of this constant vector within TOL (see test_hip_metrics_match_reference_edges)."""
    from vtamiq_amd import VTAMIQ, synth, validate
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=2))
    sd = synth.make_state_dict(m.spec, 3)
    sd["q_predictor.4.weight"] = np.zeros_like(sd["q_predictor.4.weight"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    B, N = 6, 40
    patches, pos, _ = synth.make_inputs(m.spec, B, N, 100)
    batch = (torch.linspace(0.1, 0.9, B), torch.from_numpy(patches), torch.from_numpy(pos), torch.full((B,), -1, dtype=torch.int32))
    step, corr = quiet(validate.do_validation, m, None, torch.device("cuda"), False, [batch], num_repeats=2)
    step2, pend = quiet(validate.do_validation, m, None, torch.device("cuda"), False, [batch], num_repeats=2, defer=True)
    later = quiet(pend.result)
    print(corr)
    for c in (corr, later):
        assert all(math.isnan(c[f]) for f in ("SROCC", "KROCC", "PLCC_NOFIT", "PLCC")), c
        assert math.isfinite(c["RMSE_NOFIT"]) and math.isfinite(c["RMSE"]), c
    assert step == step2 == 2 and identical(later, corr, NOFIT + ["PLCC"]) and abs(later["RMSE"] - corr["RMSE"]) <= TOL["RMSE"]
