"""The construction of tests/exact_contraction.py, proved on the CPU for every catalogue entry, so that a failure of
tests/test_gpu_exact_contraction.py can only mean the kernel: torch's hi / lo split of the fp32 operands gives exactly the intended planes,
the exactness bound holds, fp32 accumulation in three orders equals the fp64 expectation, every output plane is finite, and every
deliberately wrong contraction changes at least half of the outputs.  The last test keeps the reason for all this next to it: on Gaussian
operands a term lost in one k-step stays inside a bound relative to the tensor's maximum.  Prints the figures (pytest -s)."""
import pytest
import torch

from tests import exact_contraction as X
from tests import exact_values as E

CASES = X.catalogue()
STEP = 32                                        # the k-step of the multi-term kernels; the one-term GEMM's 64 is two of them
ROWS, COLS = 256, 64                             # the slice of a case the order and control tests work on: up to 256 x 64 outputs


def case_planes(case):
    """The intended planes of a case (fp32, CPU) and what its format is given of them."""
    dtype = X.dtype_of(case.fmt)
    ah, al, wh, wl = X.operands(dtype, case.M, case.N, case.K)
    return dtype, (ah, al, wh, wl), X.format_planes(case.fmt, ah, al, wh, wl)


def sliced(planes):
    ah, al, wh, wl = planes
    cut = lambda t, n: None if t is None else t[:n]
    return cut(ah, ROWS), cut(al, ROWS), cut(wh, COLS), cut(wl, COLS)


def test_the_catalogue_is_what_the_kernels_accept():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        t = X.TERMS[c.fmt]
        if c.entry in ("canary", "gemm", "gemm_wide", "gemm_walk"):                # include/vtamiq_hip.h vtq_k_gemm
            assert c.M % 256 == 0 and c.N % 256 == 0 and c.N <= 4096 and c.K % (128 if t == 1 else 64) == 0
        elif c.entry == "rowln":                                                   # vtq_k_gemm_rowln
            assert c.M % 128 == 0 and c.N == 768 and c.K % 32 == 0 and c.K >= 128 and t == 3
        elif c.entry == "skinny":
            assert c.K % 32 == 0 and c.K >= 32
    # the K loop shorter than, equal to and longer than the rings: the smallest K the entry takes for every format, and the engine's own
    for fmt in X.TERMS:
        ks = {c.K for c in X.cases("gemm", fmt)}
        assert {128, 256, 768, 3072, 4096} <= ks and (X.TERMS[fmt] == 1 or {64, 192} <= ks)
    # the skinny rows: both sides of every switch of launch_skinny's rule, and of 64
    for N in X.SKINNY_N:
        rows = X.skinny_rows(N)
        assert {1, 63, 64, 65} <= set(rows)
        for R in X.tail_rows.switches(N, X.tail_rows.HEAD_HORIZON):
            assert R in rows and R + 1 in rows
        assert {X.tail_rows.form(R, N) for R in rows} == X.tail_rows.possible_forms(N, X.tail_rows.HEAD_HORIZON)
    assert any(N % 16 for N in X.SKINNY_N)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_split_gives_the_intended_planes(case):
    """hi = RNE(v), lo = RNE(v - hi) on torch (the rule vtq_k_split states) of the fp32 operand hi + lo returns (hi, lo): every plane is
    non-zero somewhere, and a single-plane format sees hi alone."""
    dtype, (ah, al, wh, wl), _ = case_planes(case)
    for hi, lo in ((ah, al), (wh, wl)):
        v = hi + lo
        assert torch.equal(v.double(), hi.double() + lo.double())
        sp = E.split_expect(v, dtype, 2)
        assert torch.equal(sp[0].float(), hi) and torch.equal(sp[1].float(), lo)
        assert torch.equal(E.split_expect(v, dtype, 1)[0].float(), hi)
        assert set(hi.unique().tolist()) >= {1.0, -1.0} and set(lo.unique().tolist()) == {0.0, X.Q[dtype], -X.Q[dtype]}
        assert float(lo.abs().max()) >= 2.0 ** E.EMIN[dtype]                        # a normal number of the format
    if X.zero_pattern(dtype, case.K):
        dead = (torch.arange(case.K)[None, :] % 4) == (torch.arange(case.M)[:, None] % 4)
        assert bool((ah[dead] == 0).all()) and bool((al[dead] == 0).all()) and bool((ah[~dead] != 0).all())
    else:
        assert bool((ah != 0).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_bound_holds(case):
    """nnz (1 + 2 q) / q + |bias| / q <= 2^24 -- and with the residual update's x / (|gamma| q) on top: a condition of the case."""
    dtype, (ah, _, _, _), _ = case_planes(case)
    nnz = X.nnz_of(ah)
    assert nnz == (case.K * 3 // 4 if X.zero_pattern(dtype, case.K) else case.K)
    assert X.units(dtype, nnz, False) <= X.F32_EXACT and X.units(dtype, nnz, True) <= X.F32_EXACT, (nnz, X.units(dtype, nnz, True))
    assert float(X.bias_vector(case.N).abs().max()) <= X.BIAS_MAX and float(X.x0_matrix(ROWS, case.N).abs().max()) <= X.X0_MAX
    assert set(X.gamma_vector(768).tolist()) == set(X.GAMMAS)


def test_the_bound_is_tight_where_the_issue_says_so():
    """f16 fits up to K = 3072 and not at 4096 without the zero pattern; bf16 fits at 4096."""
    assert X.units(X.F16, 3072, False) == 12589056 + 64 * 4096 and X.units(X.F16, 3072, True) <= X.F32_EXACT
    assert X.units(X.F16, 4096, False) > X.F32_EXACT
    assert X.units(X.BF16, 4096, True) < 2.2e6


def fp32_accumulate(planes, bias, order):
    """The kernels' arithmetic on the CPU: a fp32 accumulator, one 32-wide k-step after the other in `order`, one term after the other."""
    ah, al, wh, wl = planes
    acc = bias[None, :].expand(ah.shape[0], wh.shape[0]).clone()
    terms = [(ah, wh)] + ([(al, wh)] if al is not None else []) + ([(ah, wl)] if wl is not None else [])
    for s in order:
        c = slice(s * STEP, (s + 1) * STEP)
        for a, w in terms:
            acc = acc + (a[:, c].double() @ w[:, c].double().t()).float()       # a step's own sum is below 2^6 units of q: exact
    return acc


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_fp32_accumulation_in_any_order_is_the_fp64_value(case):
    dtype, _, planes = case_planes(case)
    planes = sliced(planes)
    bias = X.bias_vector(case.N)[:COLS]
    v = X.accumulator(X.expect(*planes), bias)
    K = planes[0].shape[1]
    if K % STEP:                                                                # a padded K: zero columns up to the k-step, as the entry demands
        pad = lambda t: None if t is None else torch.cat([t, torch.zeros(t.shape[0], STEP - K % STEP)], dim=1)
        planes = tuple(pad(t) for t in planes)
    n = planes[0].shape[1] // STEP
    g = torch.Generator(device="cpu").manual_seed(X.SEED)
    for order in (range(n), range(n - 1, -1, -1), torch.randperm(n, generator=g).tolist()):
        assert torch.equal(fp32_accumulate(planes, bias, order), v)
    assert torch.equal(fp32_accumulate(planes, torch.zeros_like(bias), range(n)) + bias[None, :], v)      # the bias behind the sum
    # what the epilogues make of it: finite planes, an exact residual update
    ap = X.planes_of(case.fmt)[0]
    assert bool(torch.isfinite(E.split_expect(v, dtype, ap).float()).all())
    x0 = X.x0_matrix(case.M, case.N)[:v.shape[0], :COLS]
    for gamma in (None, X.gamma_vector(case.N)[:COLS]):
        r = X.residual(v, x0, gamma)
        assert bool(torch.isfinite(E.split_expect(r, dtype, ap).float()).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_wrong_contraction_changes_half_of_the_outputs(case):
    """The smallest K is the tightest: one 16-column half step holds about ten non-zero lo products, whose sum is zero one time in six."""
    dtype, _, planes = case_planes(case)
    planes = sliced(planes)
    K = planes[0].shape[1]
    good = X.expect(*planes)
    worst = {}
    for kind in X.WRONG_STEPPED:
        for width in (32, 16):
            for where in ("first", "middle", "last"):
                w = X.wrong(kind, *planes, X.step_columns(K, width, where))
                if w is not None:
                    share = float((w != good).double().mean())
                    worst[kind] = min(worst.get(kind, 1.0), share)
    for kind in X.WRONG_WHOLE:
        w = X.wrong(kind, *planes, None)
        if w is not None:
            worst[kind] = float((w != good).double().mean())
    print(f"{case.name}: smallest share of outputs a wrong contraction changes {worst}")
    assert "skip_step" in worst and (X.TERMS[case.fmt] < 2 or "drop_alwh" in worst)
    assert X.TERMS[case.fmt] < 3 or {"drop_ahwl", "swap_w", "add_lolo"} <= set(worst)
    for kind, share in worst.items():
        assert share >= 0.5, (kind, share)


@pytest.mark.parametrize("K", [768, 3072, 4096])
def test_a_term_lost_in_one_step_passes_the_gaussian_bound(K):
    """Why this file exists.  The Gaussian GEMM tests (tests/test_gpu_kernels.py test_gemm_bias: A ~ N(0, 1), W ~ 0.05 N(0, 1), f16 planes,
    512 x 768) bound the error by OUT_TOL = 2e-5 of the tensor's maximum.  Dropping a_lo w_hi from ONE 32-wide k-step moves the worst output
    by 5.3e-5 of the maximum at K = 768 and by 2.7e-5 / 2.4e-5 at K = 3072 / 4096: a factor 1.3 from the bound at fc2's K, so a defect half
    that size -- a 16-deep half step, one wave's fragment -- passes.  Asserted: below 3e-5 at K = 3072, where the exact operands catch it at
    nine outputs in ten; the other two K are printed."""
    g = torch.Generator(device="cpu").manual_seed(X.SEED)
    A = torch.randn(512, K, generator=g)
    W = torch.randn(768, K, generator=g) * 0.05
    a, w = E.split_expect(A, E.F16, 2).double(), E.split_expect(W, E.F16, 2).double()
    ref = X.expect(a[0], a[1], w[0], w[1])
    c = X.step_columns(K, 32, "last")
    moved = float((a[1][:, c] @ w[0][:, c].t()).abs().max() / ref.abs().max())
    print(f"Gaussian restatement K = {K}: a_lo w_hi dropped in one 32-wide step moves the worst output by {moved:.2e} of the maximum (bound 2e-5)")
    if K == 3072:
        assert moved < 3e-5
