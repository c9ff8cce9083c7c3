"""The construction of tests/exact_values.py, proved on the CPU so that a failure of tests/test_gpu_exact_values.py can only mean the kernel:
the sums are exact, the grids hold the edges they promise, a wrong conversion is told from the right one, and the fp32 restatements of the
activations have the error the code claims.  Prints E_gelu, E_sig and the edge counts (pytest -s)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import exact_values as E

DTYPES = (E.F16, E.BF16)
NAME = {E.F16: "f16", E.BF16: "bf16"}
# tests/test_gpu_kernels.py OUT_TOL: error of a 16-bit output relative to the tensor's maximum, the bound of the Gaussian GEMM tests
# (tests/test_gpu_exact_values.py asserts that this copy is the original)
OUT_TOL = {"bf16": 1e-2, "fp16": 2e-3, "bf16x3": 1e-4, "fp16x2": 2e-5, "fp16x3": 2e-5}
ATTN_S = (1, 2, 64, 128, 256)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_values(dtype, e):
    x, b = E.binade_grid(dtype, e)
    return x, b, E.acc_value(x, b)


def assert_rows_are_single_plane(x, dtype):
    sp = E.split_expect(x, dtype, 2)
    assert torch.equal(sp[0].float(), x) and bool((sp[1] == 0).all())


# ---- exact sums ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_binade_grid_sums_are_exact(dtype):
    for e in E.BINADES[dtype]:
        x, b, v = grid_values(dtype, e)
        assert_rows_are_single_plane(x, dtype)
        exact = x.double()[:, None] + b.double()[None, :]
        over = exact.abs() >= 2.0 ** 128                                       # bf16 e = 127 only: the accumulator itself overflows
        assert bool((over == torch.isinf(v)).all()) and (int(over.sum()) > 0) == (dtype == E.BF16 and e == 127)
        assert torch.equal(v.double()[~over], exact[~over]), e
        assert b.numel() == E.NCOLS and float(b.abs().max()) <= E.spacing(dtype, e)
        assert not bool(((v == 0) & torch.signbit(v)).any())                  # a zero accumulator is +0
    # the rows are ALL the format's values of the binade
    x, _ = E.binade_grid(dtype, 0)
    n = 2 ** (E.SIG_BITS[dtype] - 1)
    assert x.numel() == 2 * n + 2 and torch.equal(x[:n].to(dtype).view(torch.int16).int(), torch.arange(n, dtype=torch.int32) + int(
        torch.tensor(1.0).to(dtype).view(torch.int16)))
    assert torch.equal(x[n:2 * n], -x[:n]) and not torch.signbit(x[-2]) and bool(torch.signbit(x[-1])) and x[-1] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_activation_grid_sums_are_exact(dtype):
    x, b = E.gelu_grid(dtype)
    assert_rows_are_single_plane(x, dtype)
    v = E.acc_value(x, b)
    assert torch.equal(v.double(), x.double()[:, None] + b.double()[None, :])
    flat = v.reshape(-1).sort().values.double()
    assert float(flat[0]) == -8.0 and float(flat[-1]) < 8.0 and float((flat[1:] - flat[:-1]).max()) <= 2.0 ** -16 and v.numel() >= 2 ** 20
    assert x.numel() <= 1024 and b.numel() <= 4096 and x.numel() % 256 == 0 and b.numel() % 256 == 0
    t = E.gelu_tail(dtype)
    assert_rows_are_single_plane(t, dtype)
    assert t.numel() == 14 and torch.equal(t[7:], -t[:7]) and float(t[0]) == 8.0 and float(t[6]) >= 65504.0
    x, b = E.sigmoid_grid()
    assert_rows_are_single_plane(x, dtype)
    v = E.acc_value(x, b)
    assert torch.equal(v.double(), x.double()[:, None] + b.double()[None, :])
    assert float(v.min()) <= -104 and float(v.max()) >= 104 and int((v.abs() >= 104).sum()) > 0


# ---- edge coverage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_the_grids_hold_the_edges_they_promise(dtype):
    total = {}
    for e in E.BINADES[dtype]:
        c = E.edge_counts(grid_values(dtype, e)[2], dtype)
        print(f"edge counts {NAME[dtype]} e = {e}: {c}")
        for k, n in c.items():
            total[k] = total.get(k, 0) + n
        assert c["ties_to_even_below"] > 0 and c["ties_to_even_above"] > 0 and c["plus_zero"] > 0, e          # both parities, in every binade
        # a tie +- one fp32 ulp, and the offsets of exactly one 16-bit ulp, are present
        t, U, ks = E.offset_units(dtype, e)
        assert {0, U // 2, -(U // 2), U // 2 + 1, U // 2 - 1, -(U // 2) - 1, -(U // 2) + 1, U, -U} <= set(ks)
    print(f"edge counts {NAME[dtype]} total: {total}")
    for k in ("hi_subnormal", "hi_rounds_to_zero", "lo_underflow_to_zero", "lo_rounded", "overflow", "minus_zero_hi"):
        assert total[k] > 0, k
    if dtype == E.F16:
        assert total["lo_subnormal"] > 0                     # bf16: a lo plane below 2^-126 is a remainder below 2^-134, which rounds to zero
        v = grid_values(dtype, 15)[2]
        hi = E.split_expect(v, dtype, 1)[0].float()
        assert float(hi[v == 65504.0][0]) == 65504.0 and float(hi[v == 65519.0][0]) == 65504.0 and bool(torch.isinf(hi[v == 65520.0]).all())
        assert int((v == 65519.0).sum()) > 0 and int((v == 65520.0).sum()) > 0
        v = grid_values(dtype, -24)[2]
        assert int((v == 2.0 ** -25).sum()) > 0 and int((v == -2.0 ** -25).sum()) > 0                          # the tie that rounds to zero
        z = E.split_expect(v[v.abs() == 2.0 ** -25], dtype, 2)
        assert bool((z[0] == 0).all()) and bool((z[1] == 0).all())
        # hi normal with a subnormal lo; hi itself subnormal
        assert E.edge_counts(grid_values(dtype, -4)[2], dtype)["lo_subnormal"] > 0 and E.edge_counts(grid_values(dtype, -10)[2], dtype)["lo_subnormal"] > 0
        for e in (-15, -20, -24):
            assert E.edge_counts(grid_values(dtype, e)[2], dtype)["hi_subnormal"] > 0
    else:
        assert bool(torch.isinf(grid_values(dtype, 127)[2]).any())


# ---- separating power ------------------------------------------------------------------------------------------------------------------------
def differs(a, b):
    """per plane: elements whose bits differ (two NaNs do not)."""
    bad = (a.view(torch.int16) != b.view(torch.int16)) & ~(torch.isnan(a.float()) & torch.isnan(b.float()))
    return [int(bad[p].sum()) for p in range(a.shape[0])]


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_every_wrong_conversion_differs_where_it_claims_to(dtype):
    for kind in E.WRONG:
        seen = [0, 0]
        for e in E.BINADES[dtype]:
            v = grid_values(dtype, e)[2]
            d = differs(E.wrong_split(kind, v, dtype, 2), E.split_expect(v, dtype, 2))
            seen = [seen[0] + d[0], seen[1] + d[1]]
            d1 = differs(E.wrong_split(kind, v, dtype, 1), E.split_expect(v, dtype, 1))
            assert (d1[0] > 0) == (d[0] > 0)
        print(f"{NAME[dtype]} {kind}: differs at {seen[0]} hi and {seen[1]} lo elements of the grids")
        for p in (0, 1):
            assert (seen[p] > 0) == (p in E.WRONG_PLANES[kind]) or (kind == "flush_subnormal" and p == 1 and dtype == E.BF16), (kind, p, seen)
    # the binade the control test of the GPU file uses shows all three
    e = -10 if dtype == E.F16 else -126
    v = grid_values(dtype, e)[2]
    for kind in E.WRONG:
        assert sum(differs(E.wrong_split(kind, v, dtype, 2), E.split_expect(v, dtype, 2))) > 0, kind


@pytest.mark.parametrize("fmt", list(E.FORMAT))
def test_every_wrong_conversion_passes_the_gaussian_bound(fmt):
    """The gap this file closes: on the normal-range grids a truncating or a subnormal-flushing conversion is within OUT_TOL of the tensor's
    maximum, the bound of the Gaussian GEMM tests -- those cannot see it.  lo_of_exact is the exception in the two-plane formats: where it
    strikes it costs a whole hi ulp, more than OUT_TOL -- but it strikes at exact ties only, 2^-13 (f16) / 2^-16 (bf16) of all fp32 values,
    and the bound is relative to the tensor's maximum, so a Gaussian test sees it only when a tie falls on one of its largest elements."""
    dtype, planes = E.FORMAT[fmt]
    for e in (3,):                                   # values in [8, 16]; at e = 0 a flushed f16 lo plane (up to 2^-15 of a maximum of 2) is at the bound
        v = grid_values(dtype, e)[2]
        for kind in E.WRONG:
            w = E.wrong_split(kind, v, dtype, planes).double().sum(0)
            miss = (w - v.double()).abs()
            err = float(miss.max() / v.abs().max())
            if kind == "lo_of_exact" and planes == 2:
                assert float(miss.max()) == E.spacing(dtype, e) and bool((miss[~E.is_tie(v, dtype)] <= E.spacing(dtype, e) * 2.0 ** -8).all())
            else:
                assert err < OUT_TOL[fmt], (kind, e, err)


# ---- the activations' claims -----------------------------------------------------------------------------------------------------------------
def test_gelu_restatement_is_within_its_claim():
    err, at = E.e_gelu()
    print(f"E_gelu = {err:.3e} at x = {at:.4f} (vtamiq_amd/csrc/dev_common.h claims 2.8e-7 at x ~ 4.2)")
    assert err <= 2.8e-7 and 4.0 < abs(at) < 4.5


def test_gelu_coefficients_are_those_of_both_kernels():
    """gelu32 uses the decimal literals of gelu_erf; the hex literals of gelu_erf4's instruction block are the same fp32 numbers."""
    with open(os.path.join(ROOT, "vtamiq_amd", "csrc", "dev_common.h")) as f:
        src = f.read()
    body = src[src.index("float gelu_erf(float x)"):src.index("void gelu_erf4(")]
    lits = [float(m) for m in re.findall(r"(-?\d\.\d+(?:e-?\d+)?)f[,)]", body)]
    assert lits[0] == E.GELU_CLAMP and tuple(lits[1:8]) == E.GELU_Q, lits
    body4 = src[src.index("void gelu_erf4("):src.index("void split4_f16(")]
    assert float(re.search(r"c6 = (-?[\d.e-]+)f", body4).group(1)) == E.GELU_Q[0] and "c57 = 5.7f" in body4
    hexes = re.findall(r"v_fmaak_f32 %\d, %\d+, %\d, (0x[0-9a-f]{8})", body4)
    assert len(hexes) == 24
    for k in range(6):
        assert {int(h, 16) for h in hexes[4 * k:4 * k + 4]} == {E.GELU_Q_HEX[k]}, k
        assert int(np.float32(E.GELU_Q[k + 1]).view(np.uint32)) == E.GELU_Q_HEX[k], k


def test_gelu_tail_is_what_the_formula_does():
    """Beyond |x| = 5.7 g is held: x (1 - g) = x for x > 0 in fp32, and -|x| g, about -6.28e-9 |x|, for x < 0 where the exact result is -0."""
    g = E.gelu_tail_g()
    assert 6.2e-9 < g < 6.4e-9
    for dtype in DTYPES:
        t = E.gelu_tail(dtype).numpy()
        y = E.gelu32(t)
        assert np.array_equal(y[:7], t[:7])
        assert np.array_equal(y[7:], (t[7:].astype(np.float64) * g).astype(np.float32))
        assert float(np.abs(E.gelu64(t[7:])).max()) < 1e-14                     # the exact result there
    y = E.gelu32(np.float32([-100.0, -65504.0]))
    assert abs(y[0] + 6.3e-7) < 1e-8 and abs(y[1] + 4.1e-4) < 2e-6


def test_sigmoid_restatement():
    err, at = E.e_sig()
    print(f"E_sig = {err:.3e} at v = {at:.4f}")
    # one rounding of 1 + e (half an ulp of 1: 2^-24), one of the quotient (2^-25), the rounded argument of exp2: below 2^-23
    assert err < 2.0 ** -23
    x, b = E.sigmoid_grid()
    v = E.acc_value(x, b).numpy()
    y = E.sigmoid32(v)
    assert not np.isnan(y).any() and y.min() >= 0.0 and y.max() <= 1.0
    assert np.array_equal(y[v >= 104], np.ones_like(y[v >= 104])) and np.array_equal(y[v <= -104], np.zeros_like(y[v <= -104]))


# ---- the attention construction --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_attention_edge_vector_survives_the_sum_and_the_division(dtype):
    """Scores 0, p = 1, l = S: a query row's output is (v + zeros) / S, or 2 v / S with the spike row twice.  For S a power of two and these
    v the quotient is exact in fp32, and two planes hold v itself."""
    v = E.edge_vector(dtype, 768, True)
    assert v.unique().numel() == 768
    sp = E.split_expect(v, dtype, 2).double()
    assert torch.equal(sp[0] + sp[1], v.double())
    c = E.edge_counts(v, dtype)
    print(f"attention edge vector {NAME[dtype]}: {c}")
    assert c["ties_to_even_below"] > 0 and c["ties_to_even_above"] > 0 and c["plus_zero"] == 1
    for ka in range(3):                                      # the spike row once or twice, hi and lo products added in any order
        for kb in range(3):
            part = ka * sp[0] + kb * sp[1]
            assert torch.equal(part.float().double(), part), (ka, kb)
    for S in ATTN_S:
        inv = torch.tensor(1.0 / S)
        for mult in (1.0, 2.0):
            acc = v * mult
            assert torch.equal(acc.double(), v.double() * mult)
            assert torch.equal((acc * inv).double(), v.double() * mult / S) and bool(torch.isfinite(acc * inv).all())
    # the quotient moves values into the subnormal range of f16: conversions that round again
    if dtype == E.F16:
        q = v / 256.0
        assert E.edge_counts(q, dtype)["hi_subnormal"] > c["hi_subnormal"]


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_layernorm_edge_vector(dtype):
    for H in (768, 1024):
        b = E.edge_vector(dtype, H, False)
        assert b.unique().numel() == H and not bool(((b == 0) & torch.signbit(b)).any())
        c = E.edge_counts(b, dtype)
        print(f"LayerNorm edge vector {NAME[dtype]} H = {H}: {c}")
        for k in ("ties_to_even_below", "ties_to_even_above", "lo_rounded", "hi_subnormal", "hi_rounds_to_zero", "overflow", "minus_zero_hi"):
            assert c[k] > 0, k


def test_two_ulps_of_the_result_are_out_of_reach_for_the_gate_under_cancellation():
    """res + aux * sigmoid(v) with Gaussian res and aux: the fp32 restatement with every operation correctly rounded (one fused
    multiply-add behind sigmoid32) is thousands of ulps OF THE RESULT from fp64 where the two terms cancel, and above 2 ulps at
    thousands of elements -- while it stays within |aux| 4 E_sig + 2 ulps everywhere.  That is why tests/test_gpu_exact_values.py bounds the
    kernel with the latter."""
    x, b = E.sigmoid_grid()
    v = E.acc_value(x, b)
    res, aux = E.gate_inputs(*v.shape)
    s32 = torch.from_numpy(E.sigmoid32(v.numpy()))
    y = (res.double() + aux.double() * s32.double()).float()            # one rounding: a fused multiply-add
    ref = res.double() + aux.double() * torch.sigmoid(v.double())
    err = (y.double() - ref).abs()
    ulps = err / E.ulp32(ref)
    print(f"gate restatement: worst {float(ulps.max()):.0f} ulps of the result, {int((ulps > 2).sum())} of {ulps.numel()} elements above 2; "
          f"worst absolute error {float(err.max()):.3e}")
    assert float(ulps.max()) > 100 and int((ulps > 2).sum()) > 100
    assert bool((err <= aux.double().abs() * 4 * E.e_sig()[0] + 2 * E.ulp32(ref)).all())
