"""Every dense contraction's K loop, bit for bit, on operands whose sums are exact (tests/exact_contraction.py; tests/test_exact_contraction.py
proves the construction on the CPU): all planes non-zero, hi = +-1, lo in {0, +-q}, so every partial sum of a_hi w_hi + a_lo w_hi + a_hi w_lo in
every order is a fp32 number and the accumulator is known exactly over the whole K range.

    1  canary: one vtq_k_gemm launch per format at the smallest K returns the exact sum (if THIS fails while test_a_gemm_returns_the_exact_sum of
       tests/test_gpu_exact_values.py passes, the MFMA does not add such products the way fp32 addition would: find that out first)
    2  vtq_k_gemm: every format, every tile variant, epilogues 0 and 2 with and without gamma, every K around the ring depths and the engine's
       own; N = 4096 at K = 1024; a persistent walk of 297 tiles with chained tile boundaries and half tiles
    3  epilogue 1 (GELU) on the same exact accumulators, at the bound of test_f_gelu_is_within_its_claim
    4  vtq_k_gemm_rowln: x_f32 exact; its LayerNorm planes equal vtq_k_layernorm of the exact x
    5  vtq_k_skinny_linear: y exact, planes the stated split, epilogue 3 with gamma, at every row-count switch; the K padding contract

The operands go through the engine's own vtq_k_split and the planes read back are asserted to be the intended ones; the expectation is the
fp64 contraction of those planes, on the device.  Every element of every launch is compared.  With VTQ_CONTRACTION_TABLE=<path> in the
environment the launches, elements and misses per test and the module's wall time are written there (profiles/r22_exact_contraction.txt is one)."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from tests import exact_contraction as X
from tests import exact_values as E
from tests.gpu_util import elt_dtype, num_code, planes_of, stream, to_planes
from tests.test_gpu_exact_values import VARIANTS, bits_differ, check_bits, forced_tile, schedule_kinds, tail_reference
from vtamiq_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
TWO_PLANE = {E.F16: "fp16x3", E.BF16: "bf16x3"}          # the format whose split gives both planes of both roles
ONE_PLANE = {E.F16: "fp16", E.BF16: "bf16"}
_table = {}                                              # test -> [launches, elements compared, misses]
_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def contraction_table():
    _t0[0] = time.perf_counter()
    yield
    path = os.environ.get("VTQ_CONTRACTION_TABLE")
    if path and _table:
        wall = time.perf_counter() - _t0[0]
        with open(path, "w") as f:
            f.write(f"device: {torch.cuda.get_device_name(0)}    catalogue entries: {len(X.catalogue())}    module wall time: {wall:.1f} s\n")
            f.write("test                                   launches   elements compared   misses\n")
            for name, (n, el, miss) in _table.items():
                f.write(f"{name:<38} {n:<10} {el:<19} {miss}\n")
            f.write(f"{'total':<38} {sum(v[0] for v in _table.values()):<10} {sum(v[1] for v in _table.values()):<19} "
                    f"{sum(v[2] for v in _table.values())}\n")


class Tally:
    """The misses of one test, collected and asserted once; counts launches and elements for the table."""

    def __init__(self, name):
        self.name, self.misses, self.launches, self.elements = name, [], 0, 0

    def launched(self):
        self.launches += 1

    def check(self, got, exp, what, v=None):
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        self.elements += got.numel()
        check_bits(got, exp, what, self.misses, v)

    def done(self):
        _table[self.name] = [self.launches, self.elements, len(self.misses)]
        assert not self.misses, self.misses


# ---- operands and expectations on the device -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def device_planes(dtype, M, N, K):
    """(A planes (2, M, K), W planes (2, N, K)) of the case's fp32 operands through vtq_k_split, asserted to be the intended planes; the
    single-plane split is asserted to be the hi plane."""
    ah, al, wh, wl = X.operands(dtype, M, N, K)
    out = []
    for hi, lo, role in ((ah, al, "a"), (wh, wl, "w")):
        v = (hi + lo).to(DEV)
        p = to_planes(v, TWO_PLANE[dtype], role)
        assert p.shape[0] == 2 and torch.equal(p[0].float().cpu(), hi) and torch.equal(p[1].float().cpu(), lo)
        assert torch.equal(to_planes(v, ONE_PLANE[dtype], role)[0], p[0])
        out.append(p)
    return tuple(out)


def passed_planes(fmt, A2, W2):
    """The planes format `fmt` takes: leading planes of the two-plane tensors (the plane pitch stays that of the tensor)."""
    return A2[:planes_of(fmt, "a")], W2[:planes_of(fmt, "w")]


class Expect:
    """The exact results of one (format, operands): fp32 accumulator + bias, its planes, the residual updates.  Computed once, kept on the device."""

    def __init__(self, fmt, A, W, M, N, bias_max=X.BIAS_MAX):
        self.dtype, self.planes = elt_dtype(fmt), planes_of(fmt, "a")
        acc = X.expect(A[0], A[1] if A.shape[0] == 2 else None, W[0], W[1] if W.shape[0] == 2 else None)
        self.v = X.accumulator(acc, X.bias_vector(N, bias_max).to(DEV))
        self.x0 = X.x0_matrix(M, N).to(DEV)
        self.gamma = X.gamma_vector(N).to(DEV)
        self._kept = {}

    def split(self, which="v"):
        """planes of the accumulator ("v") or of the residual update with gamma ("gamma"): exact_values.split_expect on the CPU"""
        if which not in self._kept:
            v = self.v if which == "v" else self.resid(True)
            self._kept[which] = E.split_expect(v.cpu(), self.dtype, self.planes).to(DEV)
        return self._kept[which]

    def resid(self, use_gamma):
        if use_gamma not in self._kept:
            self._kept[use_gamma] = X.residual(self.v, self.x0, self.gamma if use_gamma else None)
        return self._kept[use_gamma]


@functools.lru_cache(maxsize=2)
def gemm_expect(fmt, M, N, K):
    A2, W2 = device_planes(elt_dtype(fmt), M, N, K)
    A, W = passed_planes(fmt, A2, W2)
    return A, W, Expect(fmt, A, W, M, N)


def ptr(t):
    return t.data_ptr() if t is not None else None


def gemm(lib, A, W, M, N, K, fmt, epi, gamma=None, x32=None, bias_max=X.BIAS_MAX):
    """vtq_k_gemm with the case's bias: -> the planes (planes, M, N) of epilogue 0 / 1, or x32 updated in place by epilogue 2."""
    bias = X.bias_vector(N, bias_max).to(DEV)
    out = torch.full((A.shape[0], M, N), 7.0, dtype=elt_dtype(fmt), device=DEV) if epi != 2 else None
    _lib.check(lib.vtq_k_gemm(A.data_ptr(), A.stride(0), K, W.data_ptr(), W.stride(0), M, N, K, num_code(fmt), epi, bias.data_ptr(), ptr(gamma),
                              ptr(x32), ptr(out), M * N, N, stream()))
    torch.cuda.synchronize()
    return x32 if epi == 2 else out


def gemm_all_epilogues(lib, t, case, variant, ex, A, W):
    """Epilogue 0 (planes) and epilogue 2 without and with gamma, every element."""
    M, N, K, fmt = case.M, case.N, case.K, case.fmt
    what = f"vtq_k_gemm {fmt} tile variant {variant} M={M} N={N} K={K}"
    t.check(gemm(lib, A, W, M, N, K, fmt, 0), ex.split(), f"{what} epilogue 0", ex.v)
    t.launched()
    for use_gamma in (False, True):
        x = gemm(lib, A, W, M, N, K, fmt, 2, ex.gamma if use_gamma else None, ex.x0.clone())
        t.check(x, ex.resid(use_gamma), f"{what} epilogue 2 gamma {use_gamma}", ex.v)
        t.launched()


# ---- 1. the canary ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(X.TERMS))
def test_1_canary_one_launch_returns_the_exact_sum(fmt):
    lib = _lib.load()
    (case,) = X.cases("canary", fmt)
    A, W, ex = gemm_expect(fmt, case.M, case.N, case.K)
    t = Tally(f"1 canary {fmt}")
    x = gemm(lib, A, W, case.M, case.N, case.K, fmt, 2, None, torch.zeros(case.M, case.N, device=DEV))
    t.launched()
    t.check(x, ex.v, f"vtq_k_gemm {fmt} tile rule M={case.M} N={case.N} K={case.K} epilogue 2 from x = 0", ex.v)
    t.done()


# ---- 2. vtq_k_gemm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(X.TERMS))
def test_2_gemm_every_k_every_tile_every_epilogue(fmt):
    lib = _lib.load()
    t = Tally(f"2 gemm {fmt}")
    for case in X.cases("gemm", fmt):
        A, W, ex = gemm_expect(fmt, case.M, case.N, case.K)
        for variant in VARIANTS:
            with forced_tile(lib, variant):
                gemm_all_epilogues(lib, t, case, variant, ex, A, W)
    t.done()


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_2_gemm_n_4096(fmt):
    lib = _lib.load()
    (case,) = X.cases("gemm_wide", fmt)
    A, W, ex = gemm_expect(fmt, case.M, case.N, case.K)
    t = Tally(f"2 gemm N=4096 {fmt}")
    for variant in VARIANTS[:2]:
        with forced_tile(lib, variant):
            gemm_all_epilogues(lib, t, case, variant, ex, A, W)
    t.done()


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_2_gemm_persistent_walk_with_chained_tiles(fmt):
    """297 tiles on 256 workgroups: every workgroup's ring runs through a tile boundary, and the lists close with half tiles (asserted)."""
    lib = _lib.load()
    (case,) = X.cases("gemm_walk", fmt)
    assert {1, 2} <= schedule_kinds(lib, case.M, case.N, case.K, fmt) and (case.M // 256) * (case.N // 256) > 256
    A, W, ex = gemm_expect(fmt, case.M, case.N, case.K)
    t = Tally(f"2 gemm walk {fmt}")
    with forced_tile(lib, VARIANTS[1]):
        gemm_all_epilogues(lib, t, case, VARIANTS[1], ex, A, W)
    t.done()


# ---- 3. GELU on the exact accumulators -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(X.TERMS))
def test_3_gelu_of_the_exact_accumulator_is_within_its_claim(fmt):
    """The bound of test_f_gelu_is_within_its_claim: 1.5 E_gelu + the output format's half ulp against fp64 for |v| < 8; against the documented
    tail (x, or -|x| g(5.7)) at 0.5 E_gelu + the half ulp beyond.  The smallest K of the format and a bias of at most 2: more than a third of the
    accumulators lie within +-8 (two thirds at K = 64), the rest reach both tails (asserted)."""
    lib = _lib.load()
    case = X.cases("gemm", fmt)[0]
    A, W, _ = gemm_expect(fmt, case.M, case.N, case.K)
    ex = Expect(fmt, A, W, case.M, case.N, X.GELU_BIAS_MAX)
    dtype, planes = E.FORMAT[fmt]
    v = ex.v.cpu().numpy()
    inner = np.abs(v) < 8.0
    assert 3 * int(inner.sum()) > v.size and int((v <= -8.0).sum()) > 0 and int((v >= 8.0).sum()) > 0
    ref = np.where(inner, E.gelu64(v), tail_reference(v))
    bound = np.where(inner, 1.5, 0.5) * E.e_gelu()[0] + E.half_ulp_last_plane(ref, dtype, planes)
    t = Tally(f"3 gelu {fmt}")
    for variant in VARIANTS:
        with forced_tile(lib, variant):
            out = gemm(lib, A, W, case.M, case.N, case.K, fmt, 1, bias_max=X.GELU_BIAS_MAX)
        t.launched()
        t.elements += v.size
        err = np.abs(out.double().sum(0).cpu().numpy() - ref)
        err = np.where(np.isnan(err), np.inf, err)
        over = err - bound
        i = int(np.argmax(over))
        print(f"measured vtq_k_gemm epilogue 1 {fmt} tile {variant} K={case.K}: worst error - bound {over.flat[i]:.3e} (error {err.flat[i]:.3e}, "
              f"bound {bound.flat[i]:.3e}) at v = {v.flat[i]:.9g}; |v| max {np.abs(v).max():.6g}, {int(inner.sum())} of {v.size} within +-8")
        if over.flat[i] > 0:
            t.misses.append(f"vtq_k_gemm {fmt} tile variant {variant} M={case.M} N={case.N} K={case.K} epilogue 1: {int((over > 0).sum())} elements over, "
                            f"first at {np.unravel_index(int(np.argmax(over > 0)), v.shape)}: error {err.flat[i]:.4e} > bound {bound.flat[i]:.4e} at v = {v.flat[i]:.9g}")
    t.done()


# ---- 4. vtq_k_gemm_rowln ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_4_rowln_updates_x_exactly_and_normalises_the_exact_x(fmt):
    lib = _lib.load()
    dtype, N = elt_dtype(fmt), X.ROWLN_N
    g = torch.Generator(device="cpu").manual_seed(X.SEED)
    ln_w, ln_b = (torch.randn(N, generator=g) + 1.0).to(DEV), torch.randn(N, generator=g).to(DEV)
    bias = X.bias_vector(N).to(DEV)
    t = Tally(f"4 rowln {fmt}")
    for case in X.cases("rowln", fmt):
        K = case.K
        A, W, ex = gemm_expect(fmt, case.M, N, K)
        for M in X.ROWLN_M:
            for use_gamma, use_ln in ((False, False), (True, False), (True, True)):
                what = f"vtq_k_gemm_rowln {fmt} M={M} K={K} gamma {use_gamma} LayerNorm {use_ln}"
                x = ex.x0[:M].clone()
                out = torch.full((2, M, N), 7.0, dtype=dtype, device=DEV) if use_ln else None
                _lib.check(lib.vtq_k_gemm_rowln(A.data_ptr(), A.stride(0), K, W.data_ptr(), W.stride(0), M, K, num_code(fmt), bias.data_ptr(),
                                                ptr(ex.gamma) if use_gamma else None, x.data_ptr(), ptr(ln_w) if use_ln else None,
                                                ptr(ln_b) if use_ln else None, ptr(out), M * N, stream()))
                torch.cuda.synchronize()
                t.launched()
                want = ex.resid(use_gamma)[:M].contiguous()
                t.check(x, want, f"{what} x_f32", ex.v[:M])
                if use_ln:
                    ln = torch.full((2, M, N), 7.0, dtype=dtype, device=DEV)
                    _lib.check(lib.vtq_k_layernorm(want.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), ln.data_ptr(), M * N, M, N, int(dtype == E.F16), 2,
                                                   stream()))
                    torch.cuda.synchronize()
                    t.check(out, ln, f"{what} planes against vtq_k_layernorm of the exact x", want)
    t.done()


# ---- 5. vtq_k_skinny_linear ------------------------------------------------------------------------------------------------------------------
GARBAGE = 3.0                                    # rows behind R and behind N, and columns behind K of a wider pitch: readable, reach no output


def skinny_operands(fmt, A2, W2, N, K, Kp, ldx):
    """xa (planes, ceil64(rows), ldx) and W (planes, ceil16(N), Kp) of the leading planes: the rows behind the operands and the columns
    [Kp, ldx) of xa hold GARBAGE, the columns [K, Kp) of the operand rows are zero."""
    A, W = passed_planes(fmt, A2, W2)
    rows = A.shape[1]
    xa = torch.full((A.shape[0], (rows + 63) // 64 * 64, ldx), GARBAGE, dtype=A.dtype, device=DEV)
    xa[:, :rows, :Kp] = 0
    xa[:, :rows, :K] = A
    wp = torch.full((W.shape[0], (N + 15) // 16 * 16, Kp), GARBAGE, dtype=W.dtype, device=DEV)
    wp[:, :N] = 0
    wp[:, :N, :K] = W
    return xa, wp


def skinny(lib, xa, wp, R, N, Kp, fmt, epi, ex):
    """-> (y fp32 (R, N), ya planes (planes, R, ceil4(N))); epilogue 3 takes the case's x0 rows and gamma."""
    bias = X.bias_vector(N).to(DEV)
    y = torch.full((R, N), float("nan"), device=DEV)
    ldya = (N + 3) // 4 * 4
    ya = torch.full((xa.shape[0], R, ldya), 7.0, dtype=xa.dtype, device=DEV)
    res = ex.x0[:R].contiguous() if epi == 3 else None
    _lib.check(lib.vtq_k_skinny_linear(xa.data_ptr(), xa.stride(0), xa.stride(1), wp.data_ptr(), wp.stride(0), R, N, Kp, num_code(fmt), epi,
                                       bias.data_ptr(), None, ptr(ex.gamma) if epi == 3 else None, ptr(res), None, N, 0, y.data_ptr(), N, N,
                                       ya.data_ptr(), R * ldya, ldya, 0, None, stream()))
    torch.cuda.synchronize()
    return y, ya


def skinny_check(lib, t, fmt, xa, wp, ex, R, N, K, Kp):
    for epi in (0, 3):
        what = f"vtq_k_skinny_linear {fmt} R={R} N={N} K={K}" + (f" padded to {Kp}" if Kp != K else "") + f" epilogue {epi}"
        y, ya = skinny(lib, xa, wp, R, N, Kp, fmt, epi, ex)
        t.launched()
        want = ex.v if epi == 0 else ex.resid(True)
        t.check(y, want[:R].contiguous(), f"{what} y", ex.v[:R])
        t.check(ya[:, :, :N], ex.split("v" if epi == 0 else "gamma")[:, :R], f"{what} planes", ex.v[:R])
        if ya.shape[2] > N and not bool((ya[:, :, N:] == 0).all()):
            t.misses.append(f"{what}: the plane columns behind N (the consumer's K padding) are not zero")


@pytest.mark.parametrize("fmt", X.SKINNY_FMTS)
def test_5_skinny_every_row_switch_every_width_every_k(fmt):
    lib = _lib.load()
    t = Tally(f"5 skinny {fmt}")
    for case in X.cases("skinny", fmt):
        N, K = case.N, case.K
        A2, W2 = device_planes(elt_dtype(fmt), case.M, N, K)
        xa, wp = skinny_operands(fmt, A2, W2, N, K, K, K)
        ex = Expect(fmt, *passed_planes(fmt, A2, W2), case.M, N)
        for R in X.skinny_rows(N):
            skinny_check(lib, t, fmt, xa, wp, ex, R, N, K, K)
    t.done()


@pytest.mark.parametrize("fmt", X.SKINNY_FMTS)
def test_5_skinny_k_padding_contract(fmt):
    """include/vtamiq_hip.h: the columns that pad K to a multiple of 32 are zero in both operands (they are multiplied); rows behind R and
    behind N, and columns behind K of a wider row pitch, are readable and reach no output."""
    lib = _lib.load()
    t = Tally(f"5 skinny padded {fmt}")
    for case, (K, Kp) in zip(X.cases("skinny_padded", fmt), X.SKINNY_PADDED_K):
        assert case.K == K
        N = case.N
        A2, W2 = device_planes(elt_dtype(fmt), case.M, N, K)
        xa, wp = skinny_operands(fmt, A2, W2, N, K, Kp, Kp + 8)
        ex = Expect(fmt, *passed_planes(fmt, A2, W2), case.M, N)
        for R in (1, 63, 65):
            skinny_check(lib, t, fmt, xa, wp, ex, R, N, K, Kp)
    t.done()


# ---- the comparison can fail -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_6_the_gpu_sum_differs_from_every_wrong_contraction(fmt):
    """One launch of (2) at the smallest K against each deliberately wrong contraction of tests/exact_contraction.py, at a 16-column half
    step: the GPU's exact sum differs from every one of them in at least half of the elements."""
    lib = _lib.load()
    case = X.cases("gemm", fmt)[0]
    A, W, ex = gemm_expect(fmt, case.M, case.N, case.K)
    x = gemm(lib, A, W, case.M, case.N, case.K, fmt, 2, None, torch.zeros(case.M, case.N, device=DEV))
    assert int(bits_differ(x, ex.v).sum()) == 0
    bias = X.bias_vector(case.N).to(DEV)
    for kind in X.WRONG_STEPPED + X.WRONG_WHOLE:
        for where in ("first", "middle", "last"):
            w = X.wrong(kind, A[0], A[1], W[0], W[1], X.step_columns(case.K, 16, where))
            share = float((x.double() != w + bias.double()[None, :]).double().mean())
            print(f"{fmt} {kind} at the {where} half step: the GPU sum differs from it at {share:.3f} of the elements")
            assert share >= 0.5, (kind, where, share)
