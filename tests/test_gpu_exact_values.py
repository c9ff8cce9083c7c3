"""Every epilogue's conversions and activations on accumulators that are exactly known (tests/exact_values.py; tests/test_exact_values.py
proves the construction on the CPU): A[i][0] = x_i, W[n][0] = 1, bias b_n, zeros elsewhere give the fp32 accumulator x_i + b_n in any order.

    a  the precondition: vtq_k_gemm epilogue 2 (every tile shape), vtq_k_skinny_linear and vtq_k_gemm_rowln return that sum BIT FOR BIT
    b  vtq_k_gemm epilogue 0, every format and tile shape, full-tile and half-tile schedule: planes bit-equal to hi = RNE(v), lo = RNE(v - hi)
    c  vtq_k_skinny_linear's plane stores (pcol0 = 0 and > 0; plain, PReLU, next_slope, the relu columns of epilogue 5)
    d  vtq_k_layernorm and vtq_k_gemm_rowln with w = 0: y = b exactly, b an edge vector; a partial last block of rows
    e  the attention kernels' O split: K = 0, V one spike row holding an edge vector, S a power of two: O = v / S exactly
    f  GELU (GEMM epilogue 1, skinny epilogue 1) against fp64 at 1.5 E_gelu + the output format's own half ulp; the two GELUs bit-identical
    g  the sigmoid gate against fp64 at 4 E_sig; exact 0 / 1 at |v| >= 104; with Gaussian res and aux at |aux| 4 E_sig + 2 fp32 ulps
    h  the control: the GPU planes differ from each deliberately wrong conversion

E_gelu and E_sig are measured from the fp32 restatements on the CPU, never from a kernel.  Rows that are f16 subnormals enter the GEMMs
prescaled (needs_prescale: the MFMA drops accumulator bits below 2^-38 when it adds the product of a subnormal operand).  With VTQ_EXACT_TABLE=<path> in the environment the
worst measured errors of f and g are written there (profiles/r16_exact_values.txt is one)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import exact_values as E
from tests import test_exact_values as CPU
from tests.gpu_util import elt_dtype, num_code, planes_of, stream
from tests.test_gpu_kernels import FMTS, OUT_TOL, TILE_256, TILE_RULE, TILE_ST
from vtamiq_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
VARIANTS = (TILE_RULE, TILE_256) + TILE_ST
_table = {}                                      # (entry, format) -> (worst error, its bound there, where)


@pytest.fixture(scope="module", autouse=True)
def exact_table():
    yield
    path = os.environ.get("VTQ_EXACT_TABLE")
    if path and _table:
        header = []
        if os.path.exists(path):
            with open(path) as f:
                for line in f:
                    if not line.startswith("#"):
                        break
                    header.append(line)
        (eg, xg), (es, vs) = E.e_gelu(), E.e_sig()
        with open(path, "w") as f:
            f.writelines(header)
            f.write(f"E_gelu = {eg:.4e} at x = {xg:.4f}    E_sig = {es:.4e} at v = {vs:.4f}    device: {torch.cuda.get_device_name(0)}\n")
            f.write("entry                         format   worst error   bound there   where\n")
            for (entry, fmt), (err, bound, where) in sorted(_table.items()):
                f.write(f"{entry:<29} {fmt:<8} {err:<13.3e} {bound:<13.3e} {where}\n")


def note(entry, fmt, err, bound, where):
    if (entry, fmt) not in _table or err > _table[(entry, fmt)][0]:
        _table[(entry, fmt)] = (err, bound, where)


def test_the_copied_bound_is_the_original():
    assert CPU.OUT_TOL == OUT_TOL and set(FMTS) == set(E.FORMAT)
    for fmt in FMTS:
        assert E.FORMAT[fmt] == (elt_dtype(fmt), planes_of(fmt, "a"))


# ---- cases and launches ----------------------------------------------------------------------------------------------------------------------
def pad(x, mult):
    """x with +0 rows behind it up to a multiple of `mult` (their accumulator is b alone)."""
    n = (x.numel() + mult - 1) // mult * mult
    return torch.cat([x, torch.zeros(n - x.numel())])


@functools.lru_cache(maxsize=None)
def binade_case(dtype, e):
    """(x padded to 256 rows, b, the accumulator on the device, name)"""
    x, b = E.binade_grid(dtype, e)
    x = pad(x, 256)
    return x, b, E.acc_value(x, b).to(DEV), f"binade e = {e}"


@functools.lru_cache(maxsize=None)
def activation_case(dtype, name):
    if name == "gelu":
        x, b = E.gelu_grid(dtype)
    elif name == "tail":
        x, b = pad(E.gelu_tail(dtype), 256), torch.zeros(256)
    else:
        x, b = E.sigmoid_grid()
    return x, b, E.acc_value(x, b).to(DEV), name


def all_cases(dtype):
    return [binade_case(dtype, e) for e in E.BINADES[dtype]] + [activation_case(dtype, n) for n in ("gelu", "tail", "sigmoid")]


def k_of(fmt):
    return 128 if planes_of(fmt, "w") == 1 and planes_of(fmt, "a") == 1 else 64


PRESCALE = 2.0 ** 10


def needs_prescale(x, fmt):
    """Rows that are f16 subnormals (the binades e < -14).  The MFMA keeps such an operand's VALUE, but adds its product at the subnormal
    exponent: accumulator bits below about 2^-38 are lost (measured on the MI355X: x_i + b_n one fp32 ulp of 2^-43 / 2^-47 short at e = -20
    / -24 in the GEMM, whose accumulators start at the bias; exact at e = -15, whose sums end at 2^-38; exact in the skinny stage, which adds
    the bias behind the MFMA -- test_a_f16_subnormal_operands_keep_their_value pins that).  The accumulator is what these tests need exact,
    so such rows enter as x 2^10 against a weight of 2^-10: both normal, the product is x."""
    nz = x[x != 0].abs()
    return elt_dtype(fmt) == E.F16 and nz.numel() > 0 and float(nz.min()) < 2.0 ** -14


def operands(x, N, fmt, K, rows=None, wrows=None, prescale=False):
    """Activation planes (rows, K) with x in column 0 and weight planes (wrows, K) with 1 in column 0 of the first N rows; lo planes zero.
    prescale: x 2^10 and 2^-10 instead (needs_prescale)."""
    dt = elt_dtype(fmt)
    sc = PRESCALE if prescale else 1.0
    A = torch.zeros((planes_of(fmt, "a"), rows or x.numel(), K), dtype=dt, device=DEV)
    A[0, :x.numel(), 0] = (x * sc).to(dt).to(DEV)
    assert torch.equal(A[0, :x.numel(), 0].float().cpu() / sc, x)
    W = torch.zeros((planes_of(fmt, "w"), wrows or N, K), dtype=dt, device=DEV)
    W[0, :N, 0] = 1.0 / sc
    return A, W


def gemm(lib, x, b, fmt, epi, prescale=None):
    """vtq_k_gemm on the case: -> (planes, M, N) of epilogue 0 / 1, or the fp32 (M, N) of epilogue 2 from x_f32 = 0, gamma = NULL."""
    M, N, K = x.numel(), b.numel(), k_of(fmt)
    A, W = operands(x, N, fmt, K, prescale=needs_prescale(x, fmt) if prescale is None else prescale)
    bias = b.to(DEV)
    out = torch.full((A.shape[0], M, N), 7.0, dtype=elt_dtype(fmt), device=DEV) if epi != 2 else None
    x32 = torch.zeros(M, N, device=DEV) if epi == 2 else None
    _lib.check(lib.vtq_k_gemm(A.data_ptr(), M * K, K, W.data_ptr(), N * K, M, N, K, num_code(fmt), epi, bias.data_ptr(), None,
                              x32.data_ptr() if epi == 2 else None, out.data_ptr() if epi != 2 else None, M * N, N, stream()))
    torch.cuda.synchronize()
    return x32 if epi == 2 else out


def skinny(lib, x, b, fmt, epi=0, want_y=True, want_ya=True, pcol0=0, post=None, nxt=None, res=None, aux=None, nsplit=0):
    """vtq_k_skinny_linear on the case (K = 32): -> (y fp32 (R, N) or None, ya planes (planes, R, N - pcol0) or None)."""
    R, N, K = x.numel(), b.numel(), 32
    Ra, Np = (R + 63) // 64 * 64, (N + 15) // 16 * 16
    A, W = operands(x, N, fmt, K, rows=Ra, wrows=Np)
    bias = b.to(DEV)
    y = torch.full((R, N), float("nan"), device=DEV) if want_y else None
    ncol = N - pcol0
    ya = torch.full((A.shape[0], R, ncol), 7.0, dtype=elt_dtype(fmt), device=DEV) if want_ya else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.vtq_k_skinny_linear(A.data_ptr(), Ra * K, K, W.data_ptr(), Np * K, R, N, K, num_code(fmt), epi, bias.data_ptr(), ptr(post), None,
                                       ptr(res), ptr(aux), N, nsplit, ptr(y), N, N, ptr(ya), R * ncol, ncol, pcol0, ptr(nxt), stream()))
    torch.cuda.synchronize()
    return y, ya


@functools.lru_cache(maxsize=None)
def expect_planes(dtype, planes, key):
    """split_expect of a case's accumulator, computed on the CPU once, kept on the device."""
    v = (binade_case(dtype, key) if isinstance(key, int) else activation_case(dtype, key))[2]
    return E.split_expect(v.cpu(), dtype, planes).to(DEV)


def bits_differ(got, exp):
    """elements whose bits differ; two NaNs count as equal (hi = inf makes lo = v - hi a NaN where v itself is inf)."""
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    return (got.view(it) != exp.view(it)) & ~(torch.isnan(got.float()) & torch.isnan(exp.float()))


def check_bits(got, exp, what, misses, v=None):
    bad = bits_differ(got, exp)
    n = int(bad.sum())
    if n:
        at = tuple(int(i) for i in bad.nonzero()[0])
        val = "" if v is None else f" v = {float(v[at[-2:]].double()):.17g}"
        misses.append(f"{what}: {n} of {bad.numel()} elements differ, first at {at}: got {float(got[at].double()):.10g} "
                      f"expected {float(exp[at].double()):.10g}{val}")
        print("MISS", misses[-1])


class forced_tile:
    def __init__(self, lib, variant):
        self.lib, self.variant = lib, variant

    def __enter__(self):
        _lib.check(self.lib.vtq_debug_gemm_variant(self.variant))

    def __exit__(self, *a):
        self.lib.vtq_debug_gemm_variant(TILE_RULE)


def schedule_kinds(lib, M, N, K, fmt):
    """the kinds (0 = 256x256 tile, 1 / 2 = its halves) in the persistent schedule of an (M, N) launch"""
    n = lib.vtq_k_gemm_schedule(M, N, K, planes_of(fmt, "w"), None, 0)
    assert n > 257
    buf = torch.zeros(n, dtype=torch.int32)
    assert lib.vtq_k_gemm_schedule(M, N, K, planes_of(fmt, "w"), buf.data_ptr(), n) == n
    return set((buf[257:] & 3).tolist())


# ---- a. the accumulator is read out exactly --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_a_gemm_returns_the_exact_sum(fmt):
    """If this fails the MFMA path does not return an exactly representable sum exactly, and nothing below is meaningful for that format."""
    lib = _lib.load()
    misses = []
    for variant in VARIANTS:
        with forced_tile(lib, variant):
            for x, b, v, name in all_cases(elt_dtype(fmt)):
                check_bits(gemm(lib, x, b, fmt, 2), v, f"tile variant {variant}, {name}", misses, v)
    assert not misses, misses


@pytest.mark.parametrize("fmt", FMTS)
def test_a_skinny_returns_the_exact_sum(fmt):
    lib = _lib.load()
    misses = []
    for x, b, v, name in all_cases(elt_dtype(fmt)):
        y, _ = skinny(lib, x, b, fmt, want_ya=False)
        check_bits(y, v, name, misses, v)
    assert not misses, misses


@pytest.mark.parametrize("fmt", ["fp16", "fp16x2", "fp16x3"])
def test_a_f16_subnormal_operands_keep_their_value(fmt):
    """vtamiq_amd/csrc/dev_common.h: "f16 subnormals are kept by the conversion and by the MFMA".  With the subnormal rows as they are (no
    prescale) the GEMM's sum is x_i + b_n to within 2^-38 -- one unit in the last place of a 24-bit sum aligned at f16's subnormal exponent
    2^-14, which is where the MFMA adds such a product (needs_prescale) -- and exact at e = -15.  A flushed operand would miss by x_i >= 2^-24."""
    lib = _lib.load()
    worst = {}
    for e in (-15, -20, -24):
        x, b, v, _ = binade_case(E.F16, e)
        for variant in (TILE_RULE, TILE_256):
            with forced_tile(lib, variant):
                d = float((gemm(lib, x, b, fmt, 2, prescale=False).double() - v.double()).abs().max())
            worst[e] = max(worst.get(e, 0.0), d)
    print(f"measured f16 subnormal operands {fmt}: max |sum - (x + b)| per binade {worst}")
    assert worst[-15] == 0.0 and worst[-20] <= 2.0 ** -38 and worst[-24] <= 2.0 ** -38, worst


def rowln(lib, x, bias, fmt, x32, ln_w, ln_b):
    """vtq_k_gemm_rowln (N = 768, K = 128) on rows x: updates x32 in place; -> the LayerNorm planes (2, M, 768) or None."""
    M, N, K = x.numel(), 768, 128
    A, W = operands(x, N, fmt, K, prescale=needs_prescale(x, fmt))
    out = torch.full((2, M, N), 7.0, dtype=elt_dtype(fmt), device=DEV) if ln_w is not None else None
    _lib.check(lib.vtq_k_gemm_rowln(A.data_ptr(), M * K, K, W.data_ptr(), N * K, M, K, num_code(fmt), bias.data_ptr(), None, x32.data_ptr(),
                                    ln_w.data_ptr() if ln_w is not None else None, ln_b.data_ptr() if ln_w is not None else None,
                                    out.data_ptr() if ln_w is not None else None, M * N, stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_a_rowln_returns_the_exact_sum(fmt):
    lib = _lib.load()
    misses = []
    dtype = elt_dtype(fmt)
    for x, b, v, name in [binade_case(dtype, e) for e in E.BINADES[dtype]] + [activation_case(dtype, "tail")]:
        x32 = torch.zeros(x.numel(), 768, device=DEV)
        rowln(lib, x, b.repeat(3).to(DEV), fmt, x32, None, None)
        check_bits(x32, v.repeat(1, 3), name, misses, v.repeat(1, 3))
    assert not misses, misses


# ---- b. the plane conversion behind every GEMM epilogue form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_b_gemm_planes_are_the_stated_split(fmt):
    """No tile shape is trimmed: test_gemm_tile_shapes_agree_bitwise compares the shapes with each other at other (M, N) and on Gaussian data,
    which says nothing about these values.  The small launches here are ALL half tiles in the forced 256x256 kernel (its schedule splits
    every tile while workgroups are idle: asserted)."""
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    misses = []
    for variant in VARIANTS:
        with forced_tile(lib, variant):
            for e in E.BINADES[dtype]:
                x, b, v, name = binade_case(dtype, e)
                check_bits(gemm(lib, x, b, fmt, 0), expect_planes(dtype, planes, e), f"tile variant {variant}, {name}", misses, v)
    assert schedule_kinds(lib, 256, 256, k_of(fmt), fmt) == {1, 2} and schedule_kinds(lib, 2304, 256, k_of(fmt), fmt) == {1, 2}
    assert not misses, misses


@pytest.mark.parametrize("fmt", FMTS)
def test_b_gemm_planes_on_whole_256_row_tiles(fmt):
    """The 256x256 kernel's whole-tile epilogue (kind 0 of vtq_k_gemm_schedule) needs more than 16 tiles per XCD, which no launch of 1024 rows
    reaches: the rows and offsets of one binade -- f16: e = -10, hi normal with a subnormal lo; bf16: e = -126 -- repeated to 2304 x 4096
    (144 tiles, all whole: asserted)."""
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    e = -10 if dtype == E.F16 else -126
    x, b = E.binade_grid(dtype, e)
    x = x.repeat(2304 // x.numel() + 1)[:2304]
    b = b.repeat(16)
    assert schedule_kinds(lib, 2304, 4096, k_of(fmt), fmt) == {0}
    v = E.acc_value(x, b)
    misses = []
    with forced_tile(lib, TILE_256):
        check_bits(gemm(lib, x, b, fmt, 0), E.split_expect(v, dtype, planes).to(DEV), f"whole tiles, e = {e}", misses, v.to(DEV))
    assert not misses, misses


# ---- c. the skinny stage's plane stores ------------------------------------------------------------------------------------------------------
def prelu(v, a):
    return torch.where(v >= 0, v, a * v)


@pytest.mark.parametrize("fmt", FMTS)
def test_c_skinny_planes_are_the_stated_split(fmt):
    """Slope 0.25: the scaling is exact (a fp32 product below 2^-126 rounds once, on the CPU as on the GPU)."""
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    slope = torch.tensor([0.25], device=DEV)
    misses = []
    for e in E.BINADES[dtype]:
        x, b, v, name = binade_case(dtype, e)
        vc = v.cpu()
        for pcol0 in (0, 64):
            _, ya = skinny(lib, x, b, fmt, want_y=False, pcol0=pcol0)
            check_bits(ya, expect_planes(dtype, planes, e)[:, :, pcol0:], f"epilogue 0, pcol0 {pcol0}, {name}", misses, v[:, pcol0:])
        act = prelu(vc, 0.25)
        want = E.split_expect(act, dtype, planes).to(DEV)
        y, ya = skinny(lib, x, b, fmt, epi=2, post=slope)
        check_bits(y, act.to(DEV), f"epilogue 2 fp32, {name}", misses, v)
        check_bits(ya, want, f"epilogue 2 planes, {name}", misses, v)
        y, ya = skinny(lib, x, b, fmt, epi=0, nxt=slope, pcol0=64)
        check_bits(y, v, f"next_slope fp32 (no activation), {name}", misses, v)
        check_bits(ya, want[:, :, 64:], f"next_slope planes, {name}", misses, v[:, 64:])
        nsplit = 128                                                   # columns >= 128: relu; planes from column 128
        y, ya = skinny(lib, x, b, fmt, epi=5, nsplit=nsplit, pcol0=nsplit)
        relu = torch.cat([vc[:, :nsplit], torch.relu(vc[:, nsplit:])], dim=1)
        check_bits(y, relu.to(DEV), f"epilogue 5 fp32, {name}", misses, v)
        check_bits(ya, E.split_expect(relu[:, nsplit:].contiguous(), dtype, planes).to(DEV), f"epilogue 5 planes, {name}", misses, v[:, nsplit:])
    assert not misses, misses


# ---- d. LayerNorm's stores -------------------------------------------------------------------------------------------------------------------
def ordinary_rows(rows, H):
    """finite rows with a spread: 0 * xhat is a zero of either sign, and +-0 + b = b for every b but -0 (which the edge vectors leave out)"""
    i = torch.arange(rows * H, dtype=torch.float32).view(rows, H)
    return (((i * 7) % 23) - 11.0) * 0.375 + 0.5


@pytest.mark.parametrize("fmt", ["bf16", "bf16x3", "fp16", "fp16x3"])
@pytest.mark.parametrize("H", [768, 1024])
def test_d_layernorm_stores_b_exactly_when_w_is_zero(fmt, H):
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    rows = 5                                                            # not a multiple of 4: the last block of rows is partial
    b = E.edge_vector(dtype, H, False)
    x = ordinary_rows(rows, H).to(DEV)
    w, bd = torch.zeros(H, device=DEV), b.to(DEV)
    out = torch.full((planes, rows + 3, H), 7.0, dtype=dtype, device=DEV)
    _lib.check(lib.vtq_k_layernorm(x.data_ptr(), w.data_ptr(), bd.data_ptr(), out.data_ptr(), (rows + 3) * H, rows, H, int(dtype == E.F16), planes,
                                   stream()))
    torch.cuda.synchronize()
    want = E.split_expect(b, dtype, planes).to(DEV)[:, None, :].expand(planes, rows, H)
    misses = []
    check_bits(out[:, :rows], want, "vtq_k_layernorm", misses, bd[None, :].expand(rows, H))
    assert bool((out[:, rows:] == 7.0).all())
    assert not misses, misses


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_d_rowln_stores_b_exactly_when_ln_w_is_zero(fmt):
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    M, H = 128, 768
    b = E.edge_vector(dtype, H, False)
    x32 = ordinary_rows(M, H).to(DEV)
    before = x32.clone()
    out = rowln(lib, torch.zeros(M), torch.zeros(H, device=DEV), fmt, x32, torch.zeros(H, device=DEV), b.to(DEV))
    assert torch.equal(x32, before)                                     # A = 0, bias = 0: the residual stream is unchanged
    want = E.split_expect(b, dtype, planes).to(DEV)[:, None, :].expand(planes, M, H)
    misses = []
    check_bits(out, want, "vtq_k_gemm_rowln", misses, b.to(DEV)[None, :].expand(M, H))
    assert not misses, misses


# ---- e. the attention kernels' output split --------------------------------------------------------------------------------------------------
ATTN_H, ATTN_NSEQ, ATTN_SLACK = 768, 3, 128


def attention_planes(v, fmt, S, spikes):
    """qkv planes (planes, 3 S + slack, 3 H): Q = 1, K = 0, V = 0 but for the rows `spikes` of every sequence, which hold v's planes."""
    dtype, planes = E.FORMAT[fmt]
    H = ATTN_H
    rows = ATTN_NSEQ * S + ATTN_SLACK
    P = torch.zeros((planes, rows, 3 * H), dtype=dtype, device=DEV)
    P[0, :, :H] = 1.0
    vp = E.split_expect(v, dtype, planes).to(DEV)
    for s in range(ATTN_NSEQ):
        for j in spikes:
            P[:, s * S + j, 2 * H:] = vp
    return P


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
def test_e_attention_output_is_the_stated_split_of_v_over_s(fmt):
    """Every score is 0, every p exactly 1, l = S: each query row's output is v / S (2 v / S with the spike row twice; 3-term formats), exact
    in fp32 for these S (tests/test_exact_values.py).  A single-plane format's V holds RNE(v): the value is that."""
    import ctypes as C
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    H = ATTN_H
    v = E.edge_vector(dtype, H, True)
    held = E.split_expect(v, dtype, planes).float().sum(0)             # what the V planes carry: v itself with two planes
    assert planes == 1 or torch.equal(held, v)
    misses = []
    try:
        for S in CPU.ATTN_S:
            layouts = [((0,), 1.0), ((S - 1,), 1.0)] if S > 1 else [((0,), 1.0)]
            if planes == 2 and S > 1:
                layouts.append(((0, S - 1), 2.0))
            for spikes, mult in layouts:
                P = attention_planes(v, fmt, S, spikes)
                rows = P.shape[1]
                o = (held * mult) * torch.tensor(1.0 / S)
                want = E.split_expect(o, dtype, planes).to(DEV)[:, None, :].expand(planes, ATTN_NSEQ * S, H)
                ov = o.to(DEV)[None, :].expand(ATTN_NSEQ * S, H)
                for entry in (0, 1, 2, "varlen"):
                    out = torch.full((planes, rows, H), 7.0, dtype=dtype, device=DEV)
                    if entry == "varlen":
                        arr = (C.c_int32 * ATTN_NSEQ)(*([S] * ATTN_NSEQ))
                        _lib.check(lib.vtq_vl_attention(P.data_ptr(), rows * 3 * H, out.data_ptr(), rows * H, ATTN_NSEQ, arr, H, num_code(fmt), stream()))
                    else:
                        _lib.check(lib.vtq_debug_attention_variant(entry))
                        _lib.check(lib.vtq_k_attention(P.data_ptr(), rows * 3 * H, out.data_ptr(), rows * H, ATTN_NSEQ, S, S, H, num_code(fmt), stream()))
                    torch.cuda.synchronize()
                    check_bits(out[:, :ATTN_NSEQ * S], want, f"entry {entry}, S = {S}, spike rows {spikes}", misses, ov)
                    if not bool((out[:, ATTN_NSEQ * S:] == 7.0).all()):
                        misses.append(f"entry {entry}, S = {S}: a row behind the sequences was stored")
    finally:
        lib.vtq_debug_attention_variant(-1)
    assert not misses, misses


# ---- f. GELU to its claim --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gelu_reference(dtype, name):
    v = activation_case(dtype, name)[2].cpu().numpy()
    return v, E.gelu64(v)


def tail_reference(v):
    """The documented tail: x for x >= 8; -|x| g(5.7) for x <= -8, where the exact result is -0."""
    return np.where(v > 0, v.astype(np.float64), v.astype(np.float64) * E.gelu_tail_g())


def gelu_misses(out, fmt, entry, v, ref, margin, misses, rows=None):
    """|value of the planes - ref| <= margin x E_gelu + half an ulp of the last plane at |ref|, per element; NaN counts as a miss."""
    dtype, planes = E.FORMAT[fmt]
    got = out.double().sum(0).cpu().numpy()
    if rows is not None:
        v, ref = v[rows], ref[rows]
    err = np.abs(got - ref)
    bound = margin * E.e_gelu()[0] + E.half_ulp_last_plane(ref, dtype, planes)
    err = np.where(np.isnan(err), np.inf, err)
    over = err - bound
    i = int(np.argmax(over))
    print(f"measured {entry} {fmt}: worst error - bound = {over.flat[i]:.3e} (error {err.flat[i]:.3e}, bound {bound.flat[i]:.3e}) at x = {v.flat[i]:.9g}; "
          f"max error {err.max():.3e}")
    note(entry, fmt, float(err.flat[i]), float(bound.flat[i]), f"x = {v.flat[i]:.9g}   (error - format's half ulp = "
         f"{float((err - (bound - margin * E.e_gelu()[0])).max()):.3e} of {margin} E_gelu = {margin * E.e_gelu()[0]:.3e}; max error {err.max():.3e})")
    if over.flat[i] > 0:
        misses.append(f"{entry}: error {err.flat[i]:.4e} > bound {bound.flat[i]:.4e} at x = {v.flat[i]:.9g} ({int((over > 0).sum())} elements)")


@pytest.mark.parametrize("fmt", FMTS)
def test_f_gelu_is_within_its_claim(fmt):
    """1.5 E_gelu: E_gelu is the restatement's own worst error against fp64 (2.79e-7); the half on top covers v_exp_f32 being within one ulp
    instead of correctly rounded (at most |x| g 2^-23 < 2.1e-8) and a true FMA against the emulated one, a tenth of what the next plausible
    defect -- a wrong degree-5 coefficient -- moves.  On the tail rows the restatement IS the documented tail, so the margin there is the
    half alone."""
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    misses = []
    x, b, _, _ = activation_case(dtype, "gelu")
    v, ref = gelu_reference(dtype, "gelu")
    xt, bt, _, _ = activation_case(dtype, "tail")
    vt = gelu_reference(dtype, "tail")[0]
    rows = torch.arange(0, x.numel(), x.numel() // 64)                  # 64 rows across [-8, 8) for the skinny stage
    outs = {}
    for variant in (TILE_RULE, TILE_256):
        with forced_tile(lib, variant):
            outs[variant] = gemm(lib, x, b, fmt, 1)
            gelu_misses(outs[variant], fmt, f"vtq_k_gemm epilogue 1 tile {variant}", v, ref, 1.5, misses)
            gelu_misses(gemm(lib, xt, bt, fmt, 1)[:, :14], fmt, f"vtq_k_gemm epilogue 1 tile {variant} tail", vt[:14], tail_reference(vt[:14]), 0.5, misses)
    _, ya = skinny(lib, x[rows], b, fmt, epi=1, want_y=False)
    gelu_misses(ya, fmt, "vtq_k_skinny_linear epilogue 1", v, ref, 1.5, misses, rows=rows.numpy())
    _, yt = skinny(lib, xt[:14], bt, fmt, epi=1, want_y=False)
    gelu_misses(yt, fmt, "vtq_k_skinny_linear epilogue 1 tail", vt[:14], tail_reference(vt[:14]), 0.5, misses)
    assert not misses, misses
    if fmt in ("fp16x3", "bf16x3", "fp16x2"):
        # vtamiq_amd/csrc/dev_common.h: gelu_erf4 runs "the same operations in the same order (bit-identical results)" as gelu_erf
        bits = []
        for variant in (TILE_RULE, TILE_256):
            check_bits(ya, outs[variant][:, rows.to(DEV)], f"skinny gelu_erf against GEMM gelu_erf4, tile {variant}", bits)
        check_bits(yt, gemm(lib, xt, bt, fmt, 1)[:, :14], "skinny gelu_erf against GEMM gelu_erf4, tail", bits)
        assert not bits, bits


# ---- g. the sigmoid gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_g_sigmoid_gate_is_within_its_claim(fmt):
    """res = 0, aux = 1: y = sigmoid(v).  4 E_sig: E_sig is the fp32 restatement's own worst error against fp64; the factor allows for the
    fast exponential (a range-reduction error of at most |v| 2^-23 relative on e^-|v|, below 0.37 x 2^-23 absolute) and the reciprocal."""
    lib = _lib.load()
    x, b, v, _ = activation_case(elt_dtype(fmt), "sigmoid")
    R, N = v.shape
    y, _ = skinny(lib, x, b, fmt, epi=4, want_ya=False, res=torch.zeros(R, N, device=DEV), aux=torch.ones(R, N, device=DEV))
    assert not bool(torch.isnan(y).any()) and float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    assert bool((y[v >= 104] == 1.0).all()) and bool((y[v <= -104] == 0.0).all())
    err = (y.double() - torch.sigmoid(v.double())).abs()
    i = int(err.argmax())
    bound = 4 * E.e_sig()[0]
    print(f"measured sigmoid gate {fmt}: {float(err.flatten()[i]):.3e} at v = {float(v.flatten()[i]):.6f} (bound {bound:.3e})")
    note("vtq_k_skinny_linear epilogue 4", fmt, float(err.flatten()[i]), bound, f"v = {float(v.flatten()[i]):.6f}")
    assert float(err.max()) <= bound


@pytest.mark.parametrize("fmt", FMTS)
def test_g_sigmoid_gate_with_gaussian_res_and_aux(fmt):
    """res + aux * sigmoid(v) with Gaussian res and aux, against fp64: |y - ref| <= |aux| 4 E_sig + 2 fp32 ulps of the fp64 value.
    The 2 ulps alone, as first written, cannot hold for ANY fp32 evaluation: the sigmoid's own error, which the test above allows 4 E_sig,
    enters multiplied by aux, and where res and aux sigmoid(v) cancel an ulp of the result is arbitrarily small.  Measured on the MI355X
    against 2 ulps alone: 2507 of 524288 elements above, the worst 3486 ulps at v = 16.449219, res = -0.267664, aux = 0.267618 (ref =
    -4.6e-5), at a worst ABSOLUTE error of 4.3e-7; the fp32 restatement with every operation correctly rounded misses it in the same way
    (tests/test_exact_values.py).  So the sigmoid keeps the allowance of the test above, scaled by |aux|, and the sum and product get the 2
    ulps.  A res or aux read from the wrong row or column misses by O(1)."""
    lib = _lib.load()
    x, b, v, _ = activation_case(elt_dtype(fmt), "sigmoid")
    R, N = v.shape
    res, aux = (t.to(DEV) for t in E.gate_inputs(R, N))
    y, _ = skinny(lib, x, b, fmt, epi=4, want_ya=False, res=res, aux=aux)
    ref = res.double() + aux.double() * torch.sigmoid(v.double())
    err = (y.double() - ref).abs()
    bound = aux.double().abs() * 4 * E.e_sig()[0] + 2 * E.ulp32(ref)
    over = err - bound
    i = int(over.argmax())
    pick = lambda t: float(t.flatten()[i])
    where = f"v = {pick(v):.6f}, res = {pick(res):.6g}, aux = {pick(aux):.6g}, ref = {pick(ref):.6g}"
    print(f"measured gate with Gaussian res, aux {fmt}: worst error - bound {pick(over):.3e} (error {pick(err):.3e}, bound {pick(bound):.3e}) at {where}; "
          f"worst absolute error {float(err.max()):.3e}; {int((err > 2 * E.ulp32(ref)).sum())} of {err.numel()} elements above 2 ulps alone")
    note("vtq_k_skinny_linear epilogue 4, Gaussian res, aux", fmt, pick(err), pick(bound), where)
    assert not bool(torch.isnan(y).any())
    assert pick(over) <= 0.0, where


# ---- h. the comparison can fail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_h_the_gpu_planes_differ_from_every_wrong_conversion(fmt):
    """One GEMM launch of (b) -- f16: e = -10, bf16: e = -126 -- against each deliberately wrong conversion: the planes differ, in the
    planes the defect touches (and equal the right one: test b)."""
    lib = _lib.load()
    dtype, planes = E.FORMAT[fmt]
    e = -10 if dtype == E.F16 else -126
    x, b, v, _ = binade_case(dtype, e)
    out = gemm(lib, x, b, fmt, 0)
    assert int(bits_differ(out, expect_planes(dtype, planes, e)).sum()) == 0
    for kind in E.WRONG:
        wrong = E.wrong_split(kind, v.cpu(), dtype, planes).to(DEV)
        n = [int(bits_differ(out[p], wrong[p]).sum()) for p in range(planes)]
        print(f"{fmt} {kind}: the GPU planes differ from it at {n} (hi, lo) elements")
        assert sum(n) >= 1, kind
        assert all(n[p] == 0 for p in range(planes) if p not in E.WRONG_PLANES[kind]), (kind, n)
