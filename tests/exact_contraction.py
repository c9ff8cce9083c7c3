"""Operands whose CONTRACTION is exactly known over the whole K range, in any summation order (no GPU code: importable anywhere).

tests/exact_values.py makes the value behind every epilogue exact with one non-zero column and zero lo planes: one k-step and one of the
up to three MFMA terms a_hi w_hi + a_lo w_hi + a_hi w_lo (vtamiq_amd/csrc/gemm.hip, "TERMS").  The K loop itself -- the DMA rings'
prologue, steady state, tile-boundary chaining and tail -- is otherwise checked on Gaussian data against a bound relative to the tensor's
maximum, which a term lost in ONE k-step stays under (tests/test_exact_contraction.py restates that).  Here every operand element is

    hi + lo,   hi in {+1, -1},   lo in {0, +q, -q},   q = 2^-12 (f16) / 2^-9 (bf16)

drawn independently for A [M][K] and W [N][K].  RNE(1 +- q) = 1 in both directions (1 - q is a tie between 1 - 2q and 1, and the even
one wins) and q is a normal number of the format, so the engine's split rule hi = RNE(v), lo = RNE(v - hi) gives exactly the planes
(+-1, lo).  Every product of the three terms is then a multiple of q, every partial sum in every order is a multiple of q below
nnz (1 + 2 q) -- nnz the largest number of non-zero A elements in a row -- and while

    nnz (1 + 2 q) / q + |bias| / q <= 2^24

every one of them is a fp32 number: the accumulator is the same whatever the order, the grouping into MFMAs or the bias-initialised start.
f16 meets that up to K = 3072; at K = 4096 row i of A is zero (both planes) in the columns k = i (mod 4), which leaves nnz = 3072.  The
bias is a small integer, x_f32 starts as small integers and gamma is drawn from {+-0.5, +-1, +-2}, so x + gamma (acc + bias) stays exact
too (units() counts its bits).  A single-plane operand sees RNE(value) = hi alone; the expectation follows from the planes actually passed.

tests/test_exact_contraction.py proves all of this on the CPU for every catalogue entry; tests/test_gpu_exact_contraction.py runs the
kernels and compares every element bit for bit."""
import collections
import functools

import torch

from tests import exact_values as E
from tests import tail_rows

F16, BF16 = E.F16, E.BF16
Q = {F16: 2.0 ** -12, BF16: 2.0 ** -9}
TERMS = {"bf16": 1, "bf16x3": 3, "fp16": 1, "fp16x2": 2, "fp16x3": 3}          # MFMAs per product (tests/gpu_util.py FORMATS)
SEED = 2203
BIAS_MAX, X0_MAX = 64, 16
GELU_BIAS_MAX = 2
GAMMAS = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
F32_EXACT = 2 ** 24

# name, entry, format, rows of A, rows of W, K.  The skinny entries hold the LARGEST row count of their width: the launches use the first R rows.
Case = collections.namedtuple("Case", "name entry fmt M N K")


def dtype_of(fmt):
    return E.FORMAT[fmt][0]


def planes_of(fmt):
    """(activation planes, weight planes) of an operand format"""
    t = TERMS[fmt]
    return (1 if t == 1 else 2), (2 if t == 3 else 1)


def zero_pattern(dtype, K):
    """f16 at K = 4096: 4096 (1 + 2 q) / q is past 2^24, so a quarter of every A row is zero."""
    return dtype == F16 and K > 3072


# ---- the draws -------------------------------------------------------------------------------------------------------------------------------
def _draw_planes(g, rows, K, q):
    hi = torch.randint(0, 2, (rows, K), generator=g, dtype=torch.int8).float() * 2.0 - 1.0
    lo = (torch.randint(0, 3, (rows, K), generator=g, dtype=torch.int8).float() - 1.0) * q
    return hi, lo


@functools.lru_cache(maxsize=3)
def operands(dtype, M, N, K):
    """(A_hi, A_lo, W_hi, W_lo) fp32 on the CPU, the INTENDED planes of A [M][K] and W [N][K]: one generator seeded by the shape, A before W.
    The fp32 operand is hi + lo (exact: 13 / 10 significand bits)."""
    g = torch.Generator(device="cpu").manual_seed(SEED + 7 * M + 11 * N + 13 * K + (0 if dtype == F16 else 1))
    ah, al = _draw_planes(g, M, K, Q[dtype])
    wh, wl = _draw_planes(g, N, K, Q[dtype])
    if zero_pattern(dtype, K):
        dead = (torch.arange(K)[None, :] % 4) == (torch.arange(M)[:, None] % 4)
        ah, al = ah.masked_fill(dead, 0.0), al.masked_fill(dead, 0.0)
    return ah, al, wh, wl


def values(dtype, M, N, K):
    """(A, W) fp32: what the engine's split (or torch's, by the same rule) is given."""
    ah, al, wh, wl = operands(dtype, M, N, K)
    return ah + al, wh + wl


def _gen(tag, n):
    return torch.Generator(device="cpu").manual_seed(SEED + 1000 * tag + n)


@functools.lru_cache(maxsize=None)
def bias_vector(N, limit=BIAS_MAX):
    """integers in [-limit, limit], fp32.  GELU_BIAS_MAX keeps two accumulators in three at K = 64 (half at K = 128) inside GELU's curved range."""
    assert limit <= BIAS_MAX
    return torch.randint(-limit, limit + 1, (N,), generator=_gen(1, N + 100000 * (BIAS_MAX - limit))).float()


@functools.lru_cache(maxsize=None)
def gamma_vector(N):
    return torch.tensor(GAMMAS)[torch.randint(0, len(GAMMAS), (N,), generator=_gen(2, N))]


@functools.lru_cache(maxsize=4)
def x0_matrix(M, N):
    """integers in [-16, 16], fp32: the residual stream before the update"""
    return torch.randint(-X0_MAX, X0_MAX + 1, (M, N), generator=_gen(3, M + N)).float()


# ---- planes and the expectation --------------------------------------------------------------------------------------------------------------
def format_planes(fmt, ah, al, wh, wl):
    """The planes format `fmt` is given, as VALUES (any float type): (A_hi, A_lo or None, W_hi, W_lo or None).  A single plane holds RNE(hi + lo) = hi."""
    ap, wp = planes_of(fmt)
    return ah, (al if ap == 2 else None), wh, (wl if wp == 2 else None)


def expect(ah, al, wh, wl):
    """The contraction the kernels state, in fp64, from the planes passed (None = the format has no such plane):
    3 terms  Ah Wh^T + Al Wh^T + Ah Wl^T   (no lo x lo product);   2 terms  (Ah + Al) W^T;   1 term  A W^T."""
    ah, wh = ah.double(), wh.double()
    acc = ah @ wh.t()
    if al is not None:
        acc = acc + al.double() @ wh.t()
    if wl is not None:
        acc = acc + ah @ wl.double().t()
    return acc


def accumulator(acc64, bias):
    """fp32 accumulator behind the epilogue: acc + bias, a zero sum being +0 (every kernel starts from +0 or from the bias).  Asserts it is exact."""
    v = acc64 + bias.double()[None, :] + 0.0
    v32 = v.float()
    assert torch.equal(v32.double(), v)
    return v32


def residual(v32, x0, gamma):
    """x0 + gamma (acc + bias) as epilogue 2 / the skinny epilogue 3 leave it, fp32; exact by the choice of x0 and gamma (asserted)."""
    r = x0.double() + (v32.double() if gamma is None else gamma.double()[None, :] * v32.double()) + 0.0
    r32 = r.float()
    assert torch.equal(r32.double(), r)
    return r32


def nnz_of(ah):
    return int((ah != 0).sum(dim=1).max())


def units(dtype, nnz, with_residual):
    """Upper bound on |any partial sum| / (its unit in the last place): nnz (1 + 2 q) / q + |bias| / q for the accumulator; the residual
    update's x + gamma v has the unit |gamma| q and adds |x| / (|gamma| q), largest at |gamma| = 1 / 2."""
    q = Q[dtype]
    u = nnz * (1.0 + 2.0 * q) / q + BIAS_MAX / q
    if with_residual:
        u += X0_MAX / (min(abs(g) for g in GAMMAS) * q)
    return u


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------
GEMM_MN = 512
GEMM_K = {1: (128, 256, 768, 3072, 4096), 2: (64, 128, 192, 256, 768, 3072, 4096), 3: (64, 128, 192, 256, 768, 3072, 4096)}
CANARY_MN = 256
WIDE = (512, 4096, 1024)                         # ViT-L fc1's N at the entry's limit
WALK = (256 * 33, 2304, 768)                     # 297 tiles of 256 x 256 on 256 workgroups: tile boundaries are chained, half tiles close the lists
ROWLN_M, ROWLN_K, ROWLN_N = (128, 384), (128, 160, 768, 3072), 768
SKINNY_FMTS = ("fp16x3", "bf16x3", "fp16x2")
SKINNY_N, SKINNY_K = (1, 48, 192, 768, 864), (32, 64, 96, 768, 3072)
SKINNY_PADDED_K = ((48, 64), (80, 96))           # (logical K, K as launched): the columns between them are zero in both operands


def skinny_rows(N):
    """1, 63, 64, 65 and both sides of every switch of launch_skinny's rows-per-workgroup rule for width N (tests/tail_rows.py)."""
    out = {1, 63, 64, 65}
    for R in tail_rows.switches(N, tail_rows.HEAD_HORIZON):
        out |= {R, R + 1}
    return sorted(out)


def gemm_k(fmt):
    return GEMM_K[TERMS[fmt]]


@functools.lru_cache(maxsize=None)
def catalogue():
    out = []
    for fmt in TERMS:
        out.append(Case(f"canary {fmt}", "canary", fmt, CANARY_MN, CANARY_MN, gemm_k(fmt)[0]))
        for K in gemm_k(fmt):
            out.append(Case(f"gemm {fmt} K={K}", "gemm", fmt, GEMM_MN, GEMM_MN, K))
    for fmt in ("fp16x3", "bf16x3"):
        out.append(Case(f"gemm wide {fmt}", "gemm_wide", fmt, *WIDE))
        out.append(Case(f"gemm walk {fmt}", "gemm_walk", fmt, *WALK))
        for K in ROWLN_K:
            out.append(Case(f"rowln {fmt} K={K}", "rowln", fmt, max(ROWLN_M), ROWLN_N, K))
    for fmt in SKINNY_FMTS:
        for N in SKINNY_N:
            for K in SKINNY_K:
                out.append(Case(f"skinny {fmt} N={N} K={K}", "skinny", fmt, skinny_rows(N)[-1], N, K))
        for K, Kp in SKINNY_PADDED_K:
            out.append(Case(f"skinny {fmt} N=192 K={K} padded to {Kp}", "skinny_padded", fmt, 65, 192, K))
    return tuple(out)


def cases(entry, fmt=None):
    return [c for c in catalogue() if c.entry == entry and (fmt is None or c.fmt == fmt)]


# ---- deliberately wrong contractions (the control of the CPU test) ---------------------------------------------------------------------------
def step_columns(K, width, where):
    """The columns of one k-step of `width` (32: a k-step of the multi-term kernels; 16: one half of it) at the first, a middle or the last step."""
    n = K // width
    s = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    return slice(s * width, (s + 1) * width)


def _z(a, b):
    return a.double() @ b.double().t()


def wrong(kind, ah, al, wh, wl, cols):
    """expect() with one defect; None where the format has nothing for it to strike.
    drop_alwh   a_lo w_hi missing in the columns `cols`        drop_ahwl   a_hi w_lo missing there
    skip_step   every term of the columns `cols` missing       swap_w      W's planes exchanged
    add_lolo    the lo x lo product added: shows that the expectation is the three-term sum and not (hi + lo)(hi + lo)"""
    good = expect(ah, al, wh, wl)
    if kind == "drop_alwh":
        return None if al is None else good - _z(al[:, cols], wh[:, cols])
    if kind == "drop_ahwl":
        return None if wl is None else good - _z(ah[:, cols], wl[:, cols])
    if kind == "skip_step":
        return good - expect(ah[:, cols], None if al is None else al[:, cols], wh[:, cols], None if wl is None else wl[:, cols])
    if kind == "swap_w":
        return None if wl is None else expect(ah, al, wl, wh)
    if kind == "add_lolo":
        return None if (al is None or wl is None) else good + _z(al, wl)
    raise ValueError(kind)


WRONG_STEPPED = ("drop_alwh", "drop_ahwl", "skip_step")
WRONG_WHOLE = ("swap_w", "add_lolo")
