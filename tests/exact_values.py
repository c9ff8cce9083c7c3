"""Inputs whose fp32 accumulator is EXACTLY known, and what every epilogue must make of it (no GPU code: importable anywhere).

Every kernel that writes 16-bit operand planes converts its fp32 result itself: the GEMM epilogues (split4_f16: hand-written v_cvt_pk +
v_fma_mix; split2; bare (T)v casts), the skinny stage's plane stores, LayerNorm's store4 and the attention kernels' O split.  On Gaussian data
and a bound relative to the tensor's maximum none of those is visible: a truncating conversion, a lo plane of the wrong sign at ties, a flushed
f16 subnormal or a wrong low-order GELU literal all pass.  The inputs made here make the value BEHIND the conversion exact:

    A[i][0] = x_i (exact in the operand format: its lo plane is zero), A[i][k > 0] = 0, W[n][0] = 1, W[n][k > 0] = 0, bias[n] = b_n

gives the accumulator x_i + b_n, and the grids keep that sum representable in fp32, so it is the same in any order, with or without the
bias-initialised accumulators.  What follows it is checked bit for bit against torch on the CPU (split_expect) or against fp64 at the
function's own claimed error (gelu32 / sigmoid32 measure that claim).  tests/test_exact_values.py proves the construction on the CPU;
tests/test_gpu_exact_values.py runs the kernels.

Zero signs: the sum of zeros of both signs is +0 under round-to-nearest, and every accumulator here adds at least one +0 product (0 x 0 of
the padding columns), so acc_value() gives x + b with -0 replaced by +0.  A NEGATIVE zero plane still occurs wherever a negative value
rounds to zero (hi = -0 at -2^-25 in f16): those are in the grids."""
import functools

import numpy as np
import torch

F16, BF16 = torch.float16, torch.bfloat16
# operand format -> (element type, planes of an ACTIVATION tensor): what the epilogues write
FORMAT = {"bf16": (BF16, 1), "bf16x3": (BF16, 2), "fp16": (F16, 1), "fp16x2": (F16, 2), "fp16x3": (F16, 2)}
SIG_BITS = {F16: 11, BF16: 8}                    # significand bits, the implicit one included
EMIN = {F16: -14, BF16: -126}                    # exponent of the smallest normal value
# f16: the normal range; hi normal with a subnormal lo; hi itself subnormal down to the 2^-25 tie that rounds to zero; 65504 / 65519 / 65520
# bf16: fp32's smallest normal binade (hi and accumulator subnormal below it), ordinary ones, and the overflow to inf at 2^128
BINADES = {F16: (0, 3, -4, -10, -14, -15, -20, -24, 15), BF16: (-126, -20, 0, 3, 60, 127)}
NCOLS = 256                                       # offsets per grid: one 256-column tile
SEED = 1611


@functools.lru_cache(maxsize=None)
def _draw():
    """The one seeded draw: NCOLS numbers in [-1, 1), shared by every grid."""
    g = torch.Generator(device="cpu").manual_seed(SEED)
    return torch.rand(NCOLS, generator=g, dtype=torch.float64) * 2.0 - 1.0


def spacing(dtype, e):
    """Distance of neighbouring `dtype` values in [2^e, 2^(e+1))."""
    return 2.0 ** (max(e, EMIN[dtype]) - (SIG_BITS[dtype] - 1))


def offset_units(dtype, e):
    """(t, U, special k): offsets are k t with t = 2^(e - 23), one fp32 ulp of the binade; U = spacing / t units make one 16-bit ulp.
    The special ones: 0, the ties +-U/2 (onto even and onto odd neighbours, as the row's significand is even or odd), a tie +- one fp32 ulp,
    +-U, the quarter points (ties of a subnormal lo plane) and U/2 - U/32 (65504 + 15 = 65519, which still rounds to 65504)."""
    t = 2.0 ** (e - 23)
    U = int(round(spacing(dtype, e) / t))
    assert U % 32 == 0
    ks = [0]
    for k in (U // 2, U // 2 + 1, U // 2 - 1, U, U - 1, 1, U // 4, U // 4 + 1, U // 4 - 1, 3 * U // 4, 3 * U // 4 + 1, 3 * U // 4 - 1,
              U // 2 - U // 32, U // 8, 3 * U // 8 + 1):
        ks += [k, -k]
    return t, U, ks


@functools.lru_cache(maxsize=None)
def binade_grid(dtype, e):
    """(x, b) fp32: rows x = every `dtype` value in [2^e, 2^(e+1)) (all 2^10 f16 / 2^7 bf16 significands; fewer where the binade is
    subnormal: 1 at f16 e = -24), their negated copies, +0 and -0; columns b = NCOLS multiples of one fp32 ulp of the binade within +- one
    16-bit ulp (bf16: the fill in steps of 2^-16 of the binade, which keeps hi + lo of most sums exact; the special offsets at fp32 ulps).
    x_i + b_n needs at most 24 significand bits (tests/test_exact_values.py)."""
    u = spacing(dtype, e)
    n0, n1 = int(round(2.0 ** e / u)), int(round(2.0 ** (e + 1) / u))
    x = torch.arange(n0, n1, dtype=torch.float64) * u
    x = torch.cat([x, -x, torch.tensor([0.0, -0.0], dtype=torch.float64)])
    t, U, ks = offset_units(dtype, e)
    q = 1 if dtype == F16 else 128
    fill = torch.round(_draw()[: NCOLS - len(ks)] * (U // q)) * q
    k = torch.cat([torch.tensor(ks, dtype=torch.float64), fill])
    assert k.numel() == NCOLS and float(k.abs().max()) <= U
    x32, b32 = x.float(), (k * t).float()
    assert torch.equal(x32.double(), x) and torch.equal(b32.double(), k * t)
    return x32, b32


@functools.lru_cache(maxsize=None)
def gelu_grid(dtype):
    """(x, b) with x + b exact, covering [-8, 8) at a spacing of 2^-17 (f16: 1024 rows of 2^-6, 2048 offsets) / 2^-16 (bf16: 256 rows of 2^-4,
    4096 offsets)."""
    step, sub = (2.0 ** -6, 2.0 ** -17) if dtype == F16 else (2.0 ** -4, 2.0 ** -16)
    x = torch.arange(-8.0, 8.0, step, dtype=torch.float64)
    b = torch.arange(0.0, step, sub, dtype=torch.float64)
    return x.float(), b.float()


GELU_TAIL = (8.0, 10.0, 20.0, 100.0, 1e3, 1e4, 65504.0)


@functools.lru_cache(maxsize=None)
def gelu_tail(dtype):
    """Tail rows +-{8, 10, 20, 100, 1e3, 1e4, 65504}, rounded to the operand format where it does not hold them (bf16: 9984, 65536); they go
    with a ZERO offset vector (65504 + 2^-17 is no fp32 number)."""
    t = torch.tensor(GELU_TAIL, dtype=torch.float32).to(dtype).float()
    return torch.cat([t, -t])


@functools.lru_cache(maxsize=None)
def sigmoid_grid():
    """(x, b): x the integers -128 .. 127 (exact in every operand format), b the multiples of 2^-11 in [0, 1): v = x + b covers [-128, 128) --
    [-104, 104] and both saturated ends -- at a spacing of 2^-11 with 19 significand bits at most."""
    return torch.arange(-128.0, 128.0, 1.0), torch.arange(0.0, 1.0, 2.0 ** -11, dtype=torch.float64).float()


def acc_value(x, b):
    """The fp32 accumulator of element (i, n): x_i + b_n, a zero sum being +0 (module docstring)."""
    return (x[:, None] + b[None, :]) + 0.0


# ---- expectations ----------------------------------------------------------------------------------------------------------------------------
def split_expect(v, dtype, planes):
    """The rule vtamiq_amd/csrc/dev_common.h states: hi = RNE(v), lo = RNE(v - hi), on torch CPU.  (planes, ...) of `dtype`.
    v = +-inf or |v| past the format: hi = +-inf and lo = v - hi = -+inf (NaN where v itself is inf), as IEEE arithmetic gives."""
    assert v.dtype == torch.float32 and v.device.type == "cpu"
    hi = v.to(dtype)
    if planes == 1:
        return hi[None]
    return torch.stack([hi, (v - hi.float()).to(dtype)])


def _toward_zero(v, dtype):
    """v truncated to `dtype` (round toward zero; a finite |v| past the largest finite value stays finite)."""
    r = v.to(dtype)
    bits = r.view(torch.int16).to(torch.int32) & 0xFFFF
    step = (r.float().abs() > v.abs()) & ~torch.isinf(v)
    bits = torch.where(step, bits - 1, bits)                 # sign-magnitude: one step toward zero, inf -> the largest finite value
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return bits.to(torch.int16).view(dtype)


def _spacing_at(a, dtype):
    """Spacing of `dtype` at the magnitudes a (float64 tensor): the distance from the largest value <= a to the next one."""
    _, ex = torch.frexp(torch.clamp(a.abs(), min=2.0 ** (EMIN[dtype] - 1)))
    return torch.pow(2.0, (torch.clamp(ex - 1, min=EMIN[dtype]) - (SIG_BITS[dtype] - 1)).double())


def is_tie(v, dtype):
    """v lies exactly half way between two neighbouring `dtype` values and rounds to a finite one (65520 -> inf is counted as overflow)."""
    d = v.double()
    below = _toward_zero(v, dtype).double().abs()
    return torch.isfinite(v.to(dtype).float()) & torch.isfinite(v) & (d.abs() - below == 0.5 * _spacing_at(below, dtype))


def wrong_split(kind, v, dtype, planes):
    """split_expect with one deliberate defect (the control tests):
    rtz              every conversion truncates instead of rounding to nearest even (both planes differ);
    lo_of_exact      lo is taken against the hi of a value a hair past v -- at an exact tie the OTHER neighbour -- while the stored hi is RNE(v):
                     the contraction / double-rounding trap the split2 comment describes, lo of the wrong sign at ties (lo plane only);
    flush_subnormal  subnormal plane values become zeros of their sign (either plane)."""
    if kind == "rtz":
        hi = _toward_zero(v, dtype)
        return hi[None] if planes == 1 else torch.stack([hi, _toward_zero(v - hi.float(), dtype)])
    good = split_expect(v, dtype, planes)
    if kind == "lo_of_exact":
        if planes == 1:
            return good
        tie = is_tie(v, dtype)
        return torch.stack([good[0], torch.where(tie, -good[1], good[1])])
    if kind == "flush_subnormal":
        sub = (good.float().abs() < 2.0 ** EMIN[dtype]) & (good.float() != 0)
        return torch.where(sub, torch.zeros_like(good) * good, good)           # 0 * x keeps the sign
    raise ValueError(kind)


WRONG = ("rtz", "lo_of_exact", "flush_subnormal")
WRONG_PLANES = {"rtz": (0, 1), "lo_of_exact": (1,), "flush_subnormal": (0, 1)}      # the planes a defect may show in


def edge_counts(v, dtype):
    """What a grid holds, counted on the fp32 values v: ties (by the parity of the neighbour RNE takes: always even -- and of the one
    truncation takes), subnormal lo planes, lo planes that underflow to zero, subnormal hi planes, overflow, zeros of both signs."""
    sp = split_expect(v, dtype, 2)
    hi, lo = sp[0].float(), sp[1].float()
    tie = is_tie(v, dtype)
    down = _toward_zero(v, dtype).float() == hi              # RNE went toward zero: the truncated neighbour is the even one
    tiny = 2.0 ** EMIN[dtype]
    rem = v.double() - hi.double()
    fin = torch.isfinite(hi)
    return {
        "ties_to_even_below": int((tie & down).sum()), "ties_to_even_above": int((tie & ~down).sum()),
        "lo_subnormal": int((fin & (lo != 0) & (lo.abs() < tiny)).sum()),
        "lo_rounded": int((fin & (lo.double() != rem) & (lo != 0)).sum()),
        "lo_underflow_to_zero": int((fin & (rem != 0) & (lo == 0)).sum()),
        "hi_subnormal": int(((hi != 0) & (hi.abs() < tiny)).sum()),
        "hi_rounds_to_zero": int(((v != 0) & (hi == 0)).sum()),
        "overflow": int(torch.isinf(hi).sum()),
        "plus_zero": int(((v == 0) & ~torch.signbit(v)).sum()), "minus_zero_hi": int(((hi == 0) & torch.signbit(hi)).sum()),
    }


# ---- fp32 restatements of the activations ----------------------------------------------------------------------------------------------------
# Q's coefficients, highest degree first: the decimal literals of gelu_erf (vtamiq_amd/csrc/dev_common.h, from tools/fit_gelu.py) ...
GELU_Q = (-4.525732038018759e-06, 1.5414956578752026e-05, 0.0005650819512084126, -0.007649366278201342, 0.05292675271630287,
          0.45905444025993347, 1.1511250734329224)
# ... and the hex literals of gelu_erf4's asm block for all but the first (which it takes from a register)
GELU_Q_HEX = (0x37814f5e, 0x3a142202, 0xbbfaa789, 0x3d58c9b9, 0x3eeb092f, 0x3f935811)
GELU_CLAMP = 5.7


def _fma32(a, b, c):
    """One FMA on fp32 arrays: the product is exact in fp64, so only the sum rounds before the rounding to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu32(v):
    """gelu_erf's formula in fp32, one rounding per FMA: max(x, 0) - |x| 2^(-1 - a Q(a)), a = min(|x|, 5.7); exp2 correctly rounded."""
    v = np.asarray(v, dtype=np.float32)
    ax = np.abs(v)
    a = np.minimum(ax, np.float32(GELU_CLAMP))
    c = [np.float32(k) for k in GELU_Q]
    q = _fma32(c[0], a, c[1])
    for k in c[2:]:
        q = _fma32(q, a, k)
    g = np.exp2(_fma32(-a, q, np.float32(-1.0)).astype(np.float64)).astype(np.float32)
    return _fma32(-ax, g, np.maximum(v, np.float32(0.0)))


def gelu_tail_g():
    """g held beyond the clamp: gelu32(x) = -|x| g for x <= -5.7 (about 6.28e-9)."""
    return float(-gelu32(np.float32(-GELU_CLAMP)) / np.float32(GELU_CLAMP))


def gelu64(v):
    """The exact-erf GELU, torch.nn.functional.gelu on float64 (the reference's transformer.py uses its default form)."""
    return torch.nn.functional.gelu(torch.as_tensor(np.asarray(v)).double()).numpy()


LOG2E32 = np.float32(1.4426950408889634)


def sigmoid32(v):
    """The skinny gate's 1 / (1 + __expf(-v)) in fp32: __expf(x) = exp2(x log2 e) with the product rounded to fp32, exp2 correctly rounded,
    then one rounded sum and one rounded division."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2((-v * LOG2E32).astype(np.float64)).astype(np.float32)
        return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


def sigmoid64(v):
    return torch.sigmoid(torch.as_tensor(np.asarray(v)).double()).numpy()


def half_ulp_last_plane(y, dtype, planes):
    """Half an ulp of the LAST plane at |y| (float64 array), per element: what the output format itself may lose.  One plane: half the spacing
    of `dtype` at |y|.  Two planes: the lo plane holds a remainder of at most half a hi spacing s, and the numbers in [s / 4, s / 2] are the
    coarsest it can be, so half the spacing there (never below half the smallest subnormal).  |y| is taken 2^-20 larger than given: the
    kernel rounds ITS fp32 value, which may lie in the binade above the reference's (this only matters beside a power of two; below 2^-20
    it adds at most 2^-31 for f16 and 2^-28 for bf16, far below the errors bounded with it)."""
    y = np.abs(np.asarray(y, dtype=np.float64)) + 2.0 ** -20
    p, emin = SIG_BITS[dtype], EMIN[dtype]

    def spacing_at(a):
        e = np.floor(np.log2(a))
        return 2.0 ** (np.maximum(e, emin) - (p - 1))
    s = spacing_at(y)
    if planes == 2:
        s = spacing_at(0.25 * s)
    return 0.5 * s


# ---- the claims, measured from the restatements (never from a kernel) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e_gelu():
    """(E_gelu, x where it is attained): max |gelu32 - gelu64| over both gelu grids."""
    best = (0.0, 0.0)
    for dtype in (F16, BF16):
        x, b = gelu_grid(dtype)
        v = (x[:, None] + b[None, :]).numpy()
        err = np.abs(gelu32(v).astype(np.float64) - gelu64(v))
        i = int(err.argmax())
        best = max(best, (float(err.flat[i]), float(v.flat[i])))
    return best


@functools.lru_cache(maxsize=None)
def e_sig():
    """(E_sig, v where it is attained): max |sigmoid32 - sigmoid64| over the sigmoid grid."""
    x, b = sigmoid_grid()
    v = (x[:, None] + b[None, :]).numpy()
    err = np.abs(sigmoid32(v).astype(np.float64) - sigmoid64(v))
    i = int(err.argmax())
    return float(err.flat[i]), float(v.flat[i])


# ---- edge vectors for the kernels without a bias to add (LayerNorm's b, the attention kernels' V row) -----------------------------------------
@functools.lru_cache(maxsize=None)
def edge_vector(dtype, n, two_plane_exact):
    """n distinct fp32 values of the binade grids, the special offsets first (0, the ties, a tie +- one fp32 ulp, +- one 16-bit ulp ...) on
    the first, second and last significand of every binade, both signs, and +0.  -0 is left out: LayerNorm's 0 * xhat + b and the attention
    kernels' sums give a zero of either sign there.
    two_plane_exact: only values that two planes of `dtype` hold exactly (hi + lo == v, finite), whose partial sums a hi + b lo (a, b in
    0 .. 2: the spike row once or twice, its products added in any order) are all fp32 numbers, and that stay exact in fp32 when divided by
    up to 256 (2^-100 <= |v| <= 2^126, or 0): what the attention kernels' V can carry."""
    cols = []
    for e in BINADES[dtype]:
        x, b = binade_grid(dtype, e)
        half = (x.numel() - 2) // 2
        rows = sorted({0, min(1, half - 1), half - 1, half, half + min(1, half - 1), 2 * half - 1, 2 * half})
        cols.append(acc_value(x[rows], b))                        # (7 or fewer rows, NCOLS)
    cand = torch.cat(cols, dim=0).t().reshape(-1)                   # offset-major: every binade's ties before anyone's fill
    cand = cand[~((cand == 0) & torch.signbit(cand))]
    if two_plane_exact:
        sp = split_expect(cand, dtype, 2).double()
        a = cand.abs()
        ok = (sp[0] + sp[1] == cand.double()) & ((cand == 0) | ((a >= 2.0 ** -100) & (a <= 2.0 ** 126)))
        for ka in range(3):
            for kb in range(3):
                part = ka * sp[0] + kb * sp[1]                      # exact in fp64: two 16-bit numbers a few binades apart
                ok &= part.float().double() == part
        cand = cand[ok]
    seen, out = set(), []
    for f in cand.tolist():
        if f not in seen:
            seen.add(f)
            out.append(f)
            if len(out) == n:
                break
    assert len(out) == n, (len(out), n)
    return torch.tensor(out, dtype=torch.float64).float()


@functools.lru_cache(maxsize=None)
def gate_inputs(R, N):
    """Gaussian res and aux of the gate test (R, N), fp32: a second seeded draw."""
    g = torch.Generator(device="cpu").manual_seed(SEED + 1)
    return torch.randn(R, N, generator=g), torch.randn(R, N, generator=g)


def ulp32(a):
    """Spacing of fp32 at |a| (float64 tensor in, float64 out)."""
    f = a.float().abs()
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()
