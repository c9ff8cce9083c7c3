"""Every kernel entry and the engine where an element index passes 2^31 (2^30 in fp32 buffers) and a byte offset 2^31 and 2^32 inside one
buffer: the shapes of tests/large_offsets.py, whose arithmetic tests/test_large_offsets_plan.py checks without a GPU.

The kernels address by (64-bit row, tile or plane base) + (32-bit offset inside a tile); one `int` row-times-pitch product among those
lines would pass every other test of the suite, which stays 15 times and more below these sizes.  The project's batch law gives the exact
reference: a row's bits do not depend on the launch it is part of, so

  reference 1  the same entry on slices of at most 16 384 rows / 64 sequences / one image of the SAME input buffers (base pointer moved,
               plane strides kept), compared bit for bit over the whole output;
  reference 2  fp64 on the first and last rows, the rows on either side of every crossed boundary and every 4097th row, at the bounds
               tests/test_gpu_kernels.py names (a slice that is itself wrong must not pass);
  canary       every output is pre-filled, so a store that went elsewhere leaves the canary at the true place, and the gaps between planes
               and behind the last row must keep it.

Inputs are seeded random data drawn on the device in slices; no compared operand holds a constant region, so a wrapped load reads other
values.  A test skips only when the device has less free memory than the catalogue says it needs.

Before the first run every expression that forms a global address or a grid size in the fourteen csrc/*.hip files and the launchers was
read for an `int` product, a uint32_t byte offset that grows with M, a narrowed count or an `int` loop variable against a 64-bit bound:
none was found that these shapes reach (row bases are int64_t, the DMA offsets cover one tile, the (int) casts of engine.hip hold row
counts that the variable-length entries bound by INT32_MAX / 4 and that the uniform ones cannot reach inside device memory), and the first
run passed.  The tests do fail on such a line: with the element index of split_kernel's store and of layernorm_kernel's load taken mod
2^31 (both land inside the buffer) test_split and test_layernorm failed in both formats, on the slice that holds the true place and on
the one that holds the wrapped one.

Measured on an MI355X (pytest --durations=0, call time; peak = torch.cuda.max_memory_allocated): the 36 tests take 16 s in all, set-up
and tear-down included, behind 17 s of process start-up that the suite pays once.  fp16x3 | the other format:
    split 0.50 | 0.02 s, 16.1 | 12.1 GiB        layernorm 0.06 | 0.02 s, 16.1 | 12.1 GiB      gemm fc1 0.41, 0.19 | 0.27, 0.07 s, 18.3 | 9.3 GiB
    gemm fc2 0.15 | 0.06 s, 14.3 | 10.3 GiB     gemm tall x 0.14 | 0.04 s, 12.6 GiB           rowln 0.03 | 0.03 s, 18.3 GiB
    attention 0.19 | 0.06 s, 13.6 | 6.9 GiB     attention varlen 0.07 | 0.06 s, 13.5 | 6.9    rollout step 0.09 | 0.05 s, 8.4 | 4.4 GiB
    rollout varlen 3.82 | 0.07 s, 8.4 | 4.4     probs 0.22 | 0.02 s, 12.0 | 10.5 GiB          cls fold 0.16 | 0.16 s, 10.2 | 10.1 GiB
    cls fold varlen 0.19 | 0.19 s, 10.3 | 10.2  images uniform 0.06 s, 13.6 GiB               images ragged / planar 0.02 s, 4.2 GiB
    engine 1.43 | 1.14 s, 2.3 GiB of tensors beside the engine's own workspace (12.0 | 7.0 GiB by vtq_workspace_bytes' formula: x 2.0,
    LayerNorm planes 2.0 | 1.0, `big` 8.0 | 4.0)
One test per run pays a one-time cost of 3 to 4 s (the rollout step here, the attention case in the run before): which one varies."""
import ctypes as C
import gc
import json

import numpy as np
import pytest
import torch

from tests import large_offsets as L
from tests.gpu_util import FORMATS, elt_dtype, num_code, planes_of, planes_value, stream, to_planes
from tests.test_gpu_kernels import ATTN_TOL, LN_TOL, OUT_TOL, RESID_TOL, _attention_ref
from tests.test_large_offsets_plan import TRANSIENT
from vtamiq_amd import VTAMIQ, _lib, synth
from vtamiq_amd import patches as patches_mod

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY16, CANARY32 = 0x7B6D, 0x7B6D7B6D          # finite in every format: fp16 60832, bf16 3.08e36, fp32 1.23e36
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
I16, I32 = torch.int16, torch.int32


# ---- the frame every test runs in ------------------------------------------------------------------------------------------------
@pytest.fixture
def mem():
    """Frees what the test held: the large tensors are locals of the test, gone when it returns (or fails)."""
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _enter(case, fmt):
    need = case.device_bytes(fmt) + TRANSIENT
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{free} bytes of device memory are free, the case {case.name} [{fmt}] needs {need}")
    torch.cuda.reset_peak_memory_stats()
    return _lib.load()


def _leave(case, fmt):
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"\n[large_offsets {case.name} {fmt}] peak {peak / 2 ** 30:.2f} GiB (catalogue {case.device_bytes(fmt) / 2 ** 30:.2f} GiB)")
    assert peak <= L.MEM_CAP, peak


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _fill_normal(t, seed, std=1.0, mean=0.0, chunk=1 << 28):
    flat, g = t.view(-1), _gen(seed)
    for i in range(0, flat.numel(), chunk):
        flat[i:i + chunk].normal_(mean, std, generator=g)
    return t


def _randn(*shape, seed, std=1.0, mean=0.0):
    return _fill_normal(torch.empty(*shape, device=DEV), seed, std, mean)


def _randn_planes(lib, rows, pitch, fmt, seed, std=1.0, slack=0):
    """[planes, rows + slack, pitch] 16-bit planes of seeded normal data, drawn and split 16 384 rows at a time."""
    npl, total = planes_of(fmt, "a"), rows + slack
    out = torch.empty((npl, total, pitch), dtype=elt_dtype(fmt), device=DEV)
    tmp, g = torch.empty((L.SLICE_ROWS, pitch), device=DEV), _gen(seed)
    for r0 in range(0, total, L.SLICE_ROWS):
        n = min(L.SLICE_ROWS, total - r0)
        tmp[:n].normal_(0.0, std, generator=g)
        _lib.check(lib.vtq_k_split(tmp.data_ptr(), out.data_ptr() + r0 * pitch * 2, total * pitch, n * pitch, FORMATS[fmt][0], npl, stream()))
    torch.cuda.synchronize()
    return out


def _canary(shape_or_numel, dtype):
    """An output buffer whose every element is the canary (16-bit and fp32 buffers, filled through the integer view)."""
    t = torch.empty(shape_or_numel, dtype=dtype, device=DEV)
    _refill(t)
    return t


def _refill(t):
    if t.element_size() == 2:
        t.view(I16).fill_(CANARY16)
    else:
        t.view(I32).fill_(CANARY32)


def _bits(t):
    return t.view(I16 if t.element_size() == 2 else I32)


def _differ(a, b, chunk=1 << 27):
    """Number of `chunk`-element pieces in which the contiguous tensors a and b differ in some bit (0: identical); no full-size temporary."""
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel() and a.element_size() == b.element_size()
    a, b = _bits(a).view(-1), _bits(b).view(-1)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for i in range(0, a.numel(), chunk):
        bad += (a[i:i + chunk] != b[i:i + chunk]).any()
    return int(bad)


def _first_difference(a, b, chunk=1 << 27):
    a, b = _bits(a).view(-1), _bits(b).view(-1)
    for i in range(0, a.numel(), chunk):
        d = (a[i:i + chunk] != b[i:i + chunk]).nonzero()
        if d.numel():
            return i + int(d[0])
    return None


def _same(a, b, what):
    if _differ(a, b):
        at = _first_difference(a, b)
        raise AssertionError(f"{what}: bits differ from the sliced launches, first at element {at} of {a.numel()}")


def _kept(t, what):
    """The canary survived in all of t."""
    v = _bits(t).reshape(-1)
    want = CANARY16 if t.element_size() == 2 else CANARY32
    bad = (v != want).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} canary elements overwritten, first at {int(bad[0])}"


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def _idx(rows):
    return torch.tensor(rows, device=DEV, dtype=torch.int64)


def _plane_views(flat, b, rows_total=None):
    """The planes of a flat output buffer laid out as Buf b says: ([plane] -> [rows, pitch] view, [plane] -> the gap behind it)."""
    rt = b.rows + b.slack_rows if rows_total is None else rows_total
    body = [flat[p * b.plane_stride: p * b.plane_stride + rt * b.pitch].view(rt, b.pitch) for p in range(b.planes)]
    gaps = [flat[p * b.plane_stride + rt * b.pitch: (p + 1) * b.plane_stride] for p in range(b.planes)]
    return body, gaps


def _value(planes, rows):
    """fp64 value of rows `rows` of a list of plane views (hi [+ lo])."""
    v = planes[0][rows].double()
    return v + planes[1][rows].double() if len(planes) == 2 else v


# ---- vtq_k_split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", L.CASES["split"].fmts)
def test_split(fmt, mem):
    """numel = 2^31 + 2^20: src passes 2^30 and 2^31 floats (4 and 8 GiB), each dst plane 2^31 elements.  The fp64 check is exact here: hi is
    the rounded value, lo the rounded remainder."""
    case = L.CASES["split"]
    lib = _enter(case, fmt)
    numel, npl, f16, dt = case.count, planes_of(fmt, "a"), FORMATS[fmt][0], elt_dtype(fmt)
    b = case.buffers(fmt)["dst"]
    src = _randn(numel, seed=101, std=3.0)
    dst = _canary(npl * b.plane_stride, dt)
    _lib.check(lib.vtq_k_split(src.data_ptr(), dst.data_ptr(), b.plane_stride, numel, f16, npl, stream()))
    body, gaps = _plane_views(dst, b)
    step = L.SLICE_ROWS * b.pitch
    ref = torch.empty((npl, step), dtype=dt, device=DEV)
    bad = 0
    for i0 in range(0, numel, step):
        n = min(step, numel - i0)
        _refill(ref)
        _lib.check(lib.vtq_k_split(src.data_ptr() + i0 * 4, ref.data_ptr(), step, n, f16, npl, stream()))
        for p in range(npl):
            bad += _differ(body[p].view(-1)[i0:i0 + n], ref[p, :n])
    assert bad == 0, f"{bad} slices of 2^24 elements differ from the sliced launches"
    for p in range(npl):
        _kept(gaps[p], f"behind plane {p}")
    rows = _idx(case.check_rows(fmt))
    xs = src.view(-1, b.pitch)[rows]
    hi = xs.to(dt)
    assert torch.equal(_bits(body[0][rows]), _bits(hi))
    if npl == 2:
        assert torch.equal(_bits(body[1][rows]), _bits((xs - hi.float()).to(dt)))
    _leave(case, fmt)


# ---- vtq_k_layernorm -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layernorm_768", "layernorm_1024"])
def test_layernorm(name, mem):
    case = L.CASES[name]
    fmt = case.fmts[0]
    lib = _enter(case, fmt)
    rows, H, npl, f16, dt = case.count, case.dims["H"], planes_of(fmt, "a"), FORMATS[fmt][0], elt_dtype(fmt)
    b = case.buffers(fmt)["out"]
    x = _randn(rows, H, seed=111, std=3.0, mean=0.7)
    w, bias = _randn(H, seed=112, mean=1.0), _randn(H, seed=113)
    out = _canary(npl * b.plane_stride, dt)
    _lib.check(lib.vtq_k_layernorm(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), b.plane_stride, rows, H, f16, npl, stream()))
    body, gaps = _plane_views(out, b)
    ref = torch.empty((npl, L.SLICE_ROWS, H), dtype=dt, device=DEV)
    bad = 0
    for r0 in range(0, rows, L.SLICE_ROWS):
        n = min(L.SLICE_ROWS, rows - r0)
        _refill(ref)
        _lib.check(lib.vtq_k_layernorm(x.data_ptr() + r0 * H * 4, w.data_ptr(), bias.data_ptr(), ref.data_ptr(), L.SLICE_ROWS * H, n, H, f16, npl,
                                       stream()))
        for p in range(npl):
            bad += _differ(body[p][r0:r0 + n], ref[p, :n])
    assert bad == 0, f"{bad} slices of 16384 rows differ from the sliced launches"
    for p in range(npl):
        _kept(gaps[p], f"behind plane {p}")
    ri = _idx(case.check_rows(fmt))
    want = torch.nn.functional.layer_norm(x[ri].double(), (H,), w.double(), bias.double(), 1e-6)
    err = _rel(_value(body, ri), want)
    print(f"[layernorm {fmt} H={H}] fp64 error {err:.3g} (bound {LN_TOL[fmt]})")
    assert err < LN_TOL[fmt], err
    _leave(case, fmt)


# ---- vtq_k_gemm ----------------------------------------------------------------------------------------------------------------
def _gemm(lib, A, a_plane, W, M, N, K, fmt, epi, bias, gamma, x, out, o_plane, a_row0=0, x_row0=0, o_row0=0):
    """vtq_k_gemm on M rows from row a_row0 of the A planes (plane stride a_plane kept), into rows from x_row0 / o_row0 of x / out."""
    _lib.check(lib.vtq_k_gemm(A.data_ptr() + a_row0 * K * 2, a_plane, K, W.data_ptr(), N * K, M, N, K, num_code(fmt), epi, bias.data_ptr(),
                              gamma.data_ptr() if gamma is not None else None, x.data_ptr() + x_row0 * N * 4 if x is not None else None,
                              out.data_ptr() + o_row0 * N * 2 if out is not None else None, o_plane, N, stream()))


@pytest.mark.parametrize("epi", L.CASES["gemm_fc1"].dims["epilogues"])
@pytest.mark.parametrize("fmt", L.CASES["gemm_fc1"].fmts)
def test_gemm_fc1_form(fmt, epi, mem):
    """M = 699 136, N = 3072, K = 768: element 2^31 of an out16 plane lies in row 699 050, byte 2^31 in row 349 525.  Every tile shape."""
    case = L.CASES["gemm_fc1"]
    lib = _enter(case, fmt)
    M, N, K, npl, dt = case.count, case.dims["N"], case.dims["K"], planes_of(fmt, "a"), elt_dtype(fmt)
    b = case.buffers(fmt)["out16"]
    A = _randn_planes(lib, M, K, fmt, seed=121)
    W, bias = to_planes(_randn(N, K, seed=122, std=0.05), fmt, "w"), _randn(N, seed=123)
    out, ref = _canary(npl * b.plane_stride, dt), _canary(npl * b.plane_stride, dt)
    for r0 in range(0, M, L.SLICE_ROWS):
        _gemm(lib, A, M * K, W, min(L.SLICE_ROWS, M - r0), N, K, fmt, epi, bias, None, None, ref, b.plane_stride, a_row0=r0, o_row0=r0)
    try:
        for tile in case.dims["tiles"]:
            _refill(out)
            _lib.check(lib.vtq_debug_gemm_variant(tile))
            _gemm(lib, A, M * K, W, M, N, K, fmt, epi, bias, None, None, out, b.plane_stride)
            _same(out, ref, f"tile shape {tile}")              # planes, gaps and all: the reference kept its canary there
    finally:
        _lib.check(lib.vtq_debug_gemm_variant(-1))
    body, gaps = _plane_views(out, b)
    for p in range(npl):
        _kept(gaps[p], f"behind plane {p}")
    ri = _idx(case.check_rows(fmt))
    pre = planes_value(A[:, ri]) @ planes_value(W).t() + bias.double()
    want = torch.nn.functional.gelu(pre) if epi == 1 else pre
    err = _rel(_value(body, ri), want)
    print(f"[gemm fc1 {fmt} epilogue {epi}] fp64 error {err:.3g} (bound {OUT_TOL[fmt]})")
    assert err < OUT_TOL[fmt], err
    _leave(case, fmt)


def _gemm_residual(name, fmt, use_gamma):
    case = L.CASES[name]
    lib = _enter(case, fmt)
    bufs = case.buffers(fmt)
    M, N, K = case.count, case.dims["N"], bufs["A"].pitch
    pad = bufs["x_f32"].slack_rows
    A = _randn_planes(lib, M, K, fmt, seed=131)
    W, bias = to_planes(_randn(N, K, seed=132, std=0.02), fmt, "w"), _randn(N, seed=133)
    gamma = _randn(N, seed=134) if use_gamma else None
    x0 = _randn(M, N, seed=135)
    ref = x0.clone()
    for r0 in range(0, M, L.SLICE_ROWS):
        _gemm(lib, A, M * K, W, min(L.SLICE_ROWS, M - r0), N, K, fmt, 2, bias, gamma, ref, None, 0, a_row0=r0, x_row0=r0)
    x = _canary((M + pad, N), torch.float32)
    try:
        for tile in case.dims["tiles"]:
            x[:M].copy_(x0)
            _lib.check(lib.vtq_debug_gemm_variant(tile))
            _gemm(lib, A, M * K, W, M, N, K, fmt, 2, bias, gamma, x, None, 0)
            _same(x[:M], ref, f"tile shape {tile}")
    finally:
        _lib.check(lib.vtq_debug_gemm_variant(-1))
    _kept(x[M:], "rows behind M")
    ri = _idx(case.check_rows(fmt, rows=M))
    h = planes_value(A[:, ri]) @ planes_value(W).t() + bias.double()
    want = x0[ri].double() + (gamma.double() * h if use_gamma else h)
    err = _rel(x[ri], want)
    print(f"[{name} {fmt} gamma={use_gamma}] fp64 error {err:.3g} (bound {RESID_TOL})")
    assert err < RESID_TOL, err
    _leave(case, fmt)


@pytest.mark.parametrize("use_gamma", [False, True])
@pytest.mark.parametrize("fmt", L.CASES["gemm_fc2"].fmts)
def test_gemm_fc2_form(fmt, use_gamma, mem):
    """M = 699 136, N = 768, K = 3072, epilogue 2: the A planes pass 2^31 elements, x_f32 2^31 bytes."""
    _gemm_residual("gemm_fc2", fmt, use_gamma)


@pytest.mark.parametrize("fmt", L.CASES["gemm_tall_x"].fmts)
def test_gemm_tall_x(fmt, mem):
    """M = 1 398 272, N = 768, the smallest K of the format: x_f32 passes 2^30 floats = 4 GiB."""
    _gemm_residual("gemm_tall_x", fmt, True)


# ---- vtq_k_gemm_rowln ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", L.CASES["rowln"].fmts)
def test_gemm_rowln(fmt, mem):
    """M = 699 136, K = 3072, LayerNorm in the epilogue; reference 1 is the two-launch path (vtq_k_gemm epilogue 2, vtq_k_layernorm) of
    tests/test_gpu_kernels.py test_gemm_rowln_is_the_two_launch_path_bit_for_bit, in slices."""
    case = L.CASES["rowln"]
    lib = _enter(case, fmt)
    bufs = case.buffers(fmt)
    M, N, K, dt, f16 = case.count, 768, case.dims["K"], elt_dtype(fmt), FORMATS[fmt][0]
    bo, pad = bufs["out16"], bufs["x_f32"].slack_rows
    A = _randn_planes(lib, M, K, fmt, seed=141)
    W, bias, gamma = to_planes(_randn(N, K, seed=142, std=0.03), fmt, "w"), _randn(N, seed=143), _randn(N, seed=144, mean=1.0)
    lw, lb = _randn(N, seed=145, mean=1.0), _randn(N, seed=146)
    x0 = _randn(M, N, seed=147, std=2.0)
    ref_x, ref16 = x0.clone(), _canary((2, M, N), dt)
    for r0 in range(0, M, L.SLICE_ROWS):
        n = min(L.SLICE_ROWS, M - r0)
        _gemm(lib, A, M * K, W, n, N, K, fmt, 2, bias, gamma, ref_x, None, 0, a_row0=r0, x_row0=r0)
        _lib.check(lib.vtq_k_layernorm(ref_x.data_ptr() + r0 * N * 4, lw.data_ptr(), lb.data_ptr(), ref16.data_ptr() + r0 * N * 2, M * N, n, N, f16, 2,
                                       stream()))
    x = _canary((M + pad, N), torch.float32)
    x[:M].copy_(x0)
    out = _canary(2 * bo.plane_stride, dt)
    _lib.check(lib.vtq_k_gemm_rowln(A.data_ptr(), M * K, K, W.data_ptr(), N * K, M, K, num_code(fmt), bias.data_ptr(), gamma.data_ptr(), x.data_ptr(),
                                    lw.data_ptr(), lb.data_ptr(), out.data_ptr(), bo.plane_stride, stream()))
    body, gaps = _plane_views(out, bo)
    _same(x[:M], ref_x, "x_f32")
    for p in range(2):
        _same(body[p], ref16[p], f"out16 plane {p}")
        _kept(gaps[p], f"behind out16 plane {p}")
    _kept(x[M:], "x_f32 rows behind M")
    ri = _idx(case.check_rows(fmt, rows=M))
    want = x0[ri].double() + gamma.double() * (planes_value(A[:, ri]) @ planes_value(W).t() + bias.double())
    ex = _rel(x[ri], want)
    eln = _rel(_value(body, ri), torch.nn.functional.layer_norm(x[ri].double(), (N,), lw.double(), lb.double(), 1e-6))
    print(f"[rowln {fmt}] fp64 error x {ex:.3g} (bound {RESID_TOL}), LayerNorm {eln:.3g} (bound {LN_TOL[fmt]})")
    assert ex < RESID_TOL and eln < LN_TOL[fmt], (ex, eln)
    _leave(case, fmt)


# ---- attention, rollout step: uniform and variable length ----------------------------------------------------------------------
def _row0(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _checked_sequences(case, fmt, row0, rows):
    """The sequences that hold a row of the fp64 check: the first and last rows, both sides of every crossing, every 4097th row."""
    return sorted({int(np.searchsorted(row0, r, side="right") - 1) for r in case.check_rows(fmt, rows=rows)})


def _attention_fp64(qkv, out, row0, seqs, H, fmt):
    """Largest error of the sequences `seqs` against fp64 attention on the same planes, relative to the largest reference value."""
    err = mx = 0.0
    for j in seqs:
        r0, S = int(row0[j]), int(row0[j + 1] - row0[j])
        want = _attention_ref(planes_value(qkv[:, r0:r0 + S]), 1, S, S, H)[0]
        got = planes_value(out[:, r0:r0 + S])
        err, mx = max(err, (got - want).abs().max().item()), max(mx, want.abs().max().item())
    return err / mx


@pytest.mark.parametrize("fmt", L.CASES["attention"].fmts)
def test_attention(fmt, mem):
    """1861 sequences of 501 rows (+ 128 slack rows): element 2^31 of a qkv plane lies in row 932 067, inside the last sequence.  All three
    kernel forms against 64-sequence launches of the library's own choice."""
    case = L.CASES["attention"]
    lib = _enter(case, fmt)
    nseq, S, H = case.count, case.dims["S"], case.dims["H"]
    bq = case.buffers(fmt)["qkv"]
    rows, total, npl, dt = bq.rows, bq.rows + bq.slack_rows, planes_of(fmt, "a"), elt_dtype(fmt)
    qkv = _randn_planes(lib, rows, 3 * H, fmt, seed=151, std=1.5, slack=bq.slack_rows)
    out, ref = _canary((npl, total, H), dt), _canary((npl, total, H), dt)
    for s0 in range(0, nseq, L.SLICE_SEQS):
        n = min(L.SLICE_SEQS, nseq - s0)
        _lib.check(lib.vtq_k_attention(qkv.data_ptr() + s0 * S * 3 * H * 2, total * 3 * H, ref.data_ptr() + s0 * S * H * 2, total * H, n, S, S, H,
                                       num_code(fmt), stream()))
    try:
        for variant in case.dims["variants"]:
            _refill(out)
            lib.vtq_debug_attention_variant(variant)
            _lib.check(lib.vtq_k_attention(qkv.data_ptr(), total * 3 * H, out.data_ptr(), total * H, nseq, S, S, H, num_code(fmt), stream()))
            _same(out, ref, f"kernel form {variant}")          # the 128 rows behind the last sequence included: canary in both
    finally:
        lib.vtq_debug_attention_variant(-1)
    _kept(out[:, rows:], "rows behind the last sequence")
    row0 = _row0([S] * nseq)
    seqs = _checked_sequences(case, fmt, row0, rows)
    err = _attention_fp64(qkv, out, row0, seqs, H, fmt)
    print(f"[attention {fmt}] fp64 error over {len(seqs)} sequences {err:.3g} (bound {ATTN_TOL[fmt]})")
    assert err < ATTN_TOL[fmt], err
    _leave(case, fmt)


@pytest.mark.parametrize("fmt", L.CASES["attention_varlen"].fmts)
def test_attention_varlen(fmt, mem):
    """1861 seeded lengths from 437 .. 565 whose sum passes row 932 068 with the last sequence.  Reference 1: vtq_k_attention on each checked
    sequence alone (the entry's own contract): the 230 or so that hold a row of the fp64 check."""
    case = L.CASES["attention_varlen"]
    lib = _enter(case, fmt)
    lengths, H = case.dims["lengths"], case.dims["H"]
    bq = case.buffers(fmt)["qkv"]
    rows, total, npl, dt, nseq = bq.rows, bq.rows + bq.slack_rows, planes_of(fmt, "a"), elt_dtype(fmt), len(lengths)
    assert rows == sum(lengths) >= L.ATT_ROWS
    qkv = _randn_planes(lib, rows, 3 * H, fmt, seed=161, std=1.5, slack=bq.slack_rows)
    out, ref = _canary((npl, total, H), dt), _canary((npl, total, H), dt)
    arr = (C.c_int32 * nseq)(*lengths)
    _lib.check(lib.vtq_vl_attention(qkv.data_ptr(), total * 3 * H, out.data_ptr(), total * H, nseq, arr, H, num_code(fmt), stream()))
    row0 = _row0(lengths)
    seqs = _checked_sequences(case, fmt, row0, rows)
    assert len(seqs) >= 64 and nseq - 1 in seqs
    for j in seqs:
        r0, S = int(row0[j]), lengths[j]
        _lib.check(lib.vtq_k_attention(qkv.data_ptr() + r0 * 3 * H * 2, total * 3 * H, ref.data_ptr() + r0 * H * 2, total * H, 1, S, S, H, num_code(fmt),
                                       stream()))
    torch.cuda.synchronize()
    for j in seqs:
        r0, S = int(row0[j]), lengths[j]
        assert torch.equal(_bits(out[:, r0:r0 + S]), _bits(ref[:, r0:r0 + S])), f"sequence {j} (rows {r0} .. {r0 + S})"
    _kept(out[:, rows:], "rows behind the last sequence")
    written = (_bits(out[0, :rows, :8]) != CANARY16).any(dim=1)
    assert bool(written.all()), f"{int((~written).sum())} rows were never stored"
    err = _attention_fp64(qkv, out, row0, seqs, H, fmt)
    print(f"[attention varlen {fmt}] fp64 error {err:.3g} (bound {ATTN_TOL[fmt]})")
    assert err < ATTN_TOL[fmt], err
    _leave(case, fmt)


def _rollout_fp64(qkv, r_in, row0, j, H):
    """One rollout step of sequence j in fp64: 1/2 r + 1/(2 h) sum_head r^T softmax(Q K^T / 8)."""
    r0, S, nh = int(row0[j]), int(row0[j + 1] - row0[j]), H // 64
    v = planes_value(qkv[:, r0:r0 + S, :2 * H]).reshape(S, 2, nh, 64)
    q, k = v[:, 0].permute(1, 0, 2), v[:, 1].permute(1, 0, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)                 # [head, query, key]
    r = r_in[r0:r0 + S].double()
    return 0.5 * r + (r @ p).sum(0) / (2 * nh)


def _rollout(name, fmt):
    case = L.CASES[name]
    lib = _enter(case, fmt)
    H, S = case.dims["H"], case.dims["S"]
    lengths = case.dims.get("lengths") or [S] * case.count
    bufs = case.buffers(fmt)
    bq, nseq = bufs["qkv"], len(lengths)
    rows, total = bq.rows, bq.rows + bq.slack_rows
    qkv = _randn_planes(lib, rows, 3 * H, fmt, seed=171, std=1.5, slack=bq.slack_rows)
    r_in = torch.empty(rows, device=DEV).uniform_(0.1, 1.0, generator=_gen(172))
    part = torch.empty(bufs["part"].numel, device=DEV)
    r_out, ref = _canary(rows + L.GAP, torch.float32), _canary(rows + L.GAP, torch.float32)
    row0 = _row0(lengths)
    step = lambda r0, n, S_, dst: _lib.check(lib.vtq_k_rollout_step(qkv.data_ptr() + r0 * 3 * H * 2, total * 3 * H, r_in.data_ptr() + r0 * 4,
                                                                     dst.data_ptr() + r0 * 4, part.data_ptr(), n, S_, S_, H, num_code(fmt), 0, stream()))
    if "lengths" in case.dims:
        arr = (C.c_int32 * nseq)(*lengths)
        _lib.check(lib.vtq_vl_rollout_step(qkv.data_ptr(), total * 3 * H, r_in.data_ptr(), r_out.data_ptr(), part.data_ptr(), nseq, arr, H,
                                           num_code(fmt), 0, stream()))
        seqs = _checked_sequences(case, fmt, row0, rows)
        assert len(seqs) >= 64
        for j in seqs:                                                    # the sequence alone: the entry's own contract
            step(int(row0[j]), 1, lengths[j], ref)
        torch.cuda.synchronize()
        for j in seqs:
            a, e = int(row0[j]), int(row0[j + 1])
            assert torch.equal(_bits(r_out[a:e]), _bits(ref[a:e])), f"sequence {j} (rows {a} .. {e})"
        assert bool((_bits(r_out[:rows]) != CANARY32).all()), "an output was never stored"
    else:
        step(0, nseq, S, r_out)
        for s0 in range(0, nseq, L.SLICE_SEQS):
            step(s0 * S, min(L.SLICE_SEQS, nseq - s0), S, ref)
        _same(r_out, ref, "r_out")
        seqs = _checked_sequences(case, fmt, row0, rows)
    _kept(r_out[rows:], "behind r_out")
    err = mx = 0.0
    for j in seqs:
        want = _rollout_fp64(qkv, r_in, row0, j, H)
        got = r_out[int(row0[j]):int(row0[j + 1])].double()
        err, mx = max(err, (got - want).abs().max().item()), max(mx, want.abs().max().item())
    print(f"[{name} {fmt}] fp64 error {err / mx:.3g} (bound {ATTN_TOL[fmt]})")
    assert err / mx < ATTN_TOL[fmt], err / mx
    _leave(case, fmt)


@pytest.mark.parametrize("fmt", L.CASES["rollout_step"].fmts)
def test_rollout_step(fmt, mem):
    """vtq_k_rollout_step on the attention case's QKV planes."""
    _rollout("rollout_step", fmt)


@pytest.mark.parametrize("fmt", L.CASES["rollout_step_varlen"].fmts)
def test_rollout_step_varlen(fmt, mem):
    """vtq_vl_rollout_step on the variable-length attention case's QKV planes."""
    _rollout("rollout_step_varlen", fmt)


# ---- vtq_k_attention_probs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", L.CASES["probs"].fmts)
def test_attention_probs(fmt, mem):
    """713 sequences of 501 rows, 12 heads: probs passes 2^30 floats in sequence 356 and 2^31 floats in the last one."""
    case = L.CASES["probs"]
    lib = _enter(case, fmt)
    nseq, S, H = case.count, case.dims["S"], case.dims["H"]
    nh, per = H // 64, (H // 64) * S * S
    bp = case.buffers(fmt)["probs"]
    assert bp.numel == nseq * per
    qkv = _randn_planes(lib, nseq * S, 3 * H, fmt, seed=181, std=1.5)
    probs = _canary(bp.numel + L.GAP, torch.float32)
    _lib.check(lib.vtq_k_attention_probs(qkv.data_ptr(), nseq * S * 3 * H, probs.data_ptr(), nseq, S, S, H, num_code(fmt), 0, stream()))
    ref = torch.empty(L.SLICE_SEQS * per, device=DEV)
    bad = 0
    for s0 in range(0, nseq, L.SLICE_SEQS):
        n = min(L.SLICE_SEQS, nseq - s0)
        _refill(ref)
        _lib.check(lib.vtq_k_attention_probs(qkv.data_ptr() + s0 * S * 3 * H * 2, nseq * S * 3 * H, ref.data_ptr(), n, S, S, H, num_code(fmt), 0,
                                             stream()))
        bad += _differ(probs[s0 * per:(s0 + n) * per], ref[:n * per])
    assert bad == 0, f"{bad} pieces differ from the 64-sequence launches"
    _kept(probs[bp.numel:], "behind probs")
    # fp64: rows of S probabilities -- (sequence, head, query) -- first, last, beside both crossings, every 4097th
    rows = _idx(case.check_rows(fmt))
    seq, head, qi = rows // (nh * S), (rows // S) % nh, rows % S
    key_rows = (seq * S)[:, None] + torch.arange(S, device=DEV)[None, :]
    table = probs[:bp.numel].view(-1, S)
    err = 0.0
    for h in range(nh):
        m = head == h
        if not bool(m.any()):
            continue
        k = planes_value(qkv[:, :, H + 64 * h:H + 64 * h + 64][:, key_rows[m]])               # [n, S, 64]
        q = planes_value(qkv[:, :, 64 * h:64 * h + 64][:, (seq * S + qi)[m]])                 # [n, 64]
        want = torch.softmax((k @ q[:, :, None])[:, :, 0] / 8.0, dim=-1)
        err = max(err, (table[rows[m]].double() - want).abs().max().item() / want.max().item())
    print(f"[probs {fmt}] fp64 error over {rows.numel()} rows {err:.3g} (bound {ATTN_TOL[fmt]})")
    assert err < ATTN_TOL[fmt], err
    _leave(case, fmt)


# ---- vtq_k_cls_fold, vtq_vl_cls_fold ---------------------------------------------------------------------------------------------
def _fold_fp64(x, q, W64, bqkv, lw, lb, r0, S, H):
    """ctx of one sequence by the un-folded formula in fp64: softmax(q_h . K_h / 8) V_h with K, V projected from LayerNorm(x)."""
    nh = H // 64
    ln = torch.nn.functional.layer_norm(x[r0:r0 + S].double(), (H,), lw.double(), lb.double(), 1e-6)
    k = (ln @ W64[H:2 * H].t() + bqkv[H:2 * H].double()).view(S, nh, 64).permute(1, 0, 2)
    v = (ln @ W64[2 * H:].t() + bqkv[2 * H:].double()).view(S, nh, 64).permute(1, 0, 2)
    p = torch.softmax((k @ q.double().view(nh, 64, 1))[:, :, 0] / 8.0, dim=-1)               # [head, S]
    return (p[:, None, :] @ v)[:, 0].reshape(H)


def _cls_fold(name, fmt):
    case = L.CASES[name]
    lib = _enter(case, fmt)
    assert lib.vtq_k_cls_fold_chunk_rows() == L.CHUNK_ROWS
    H, S, nseq = case.dims["H"], case.dims["S"], case.count
    lengths = case.dims.get("lengths") or [S] * nseq
    bufs = case.buffers(fmt)
    rows, nh, dt, apl = bufs["x"].rows, H // 64, elt_dtype(fmt), planes_of(fmt, "a")
    row0 = _row0(lengths)
    x = _randn(rows, H, seed=191, std=2.0, mean=0.3)
    q = _randn(nseq, H, seed=192)
    Wp, bqkv = to_planes(_randn(3 * H, H, seed=193, std=0.05), fmt, "w"), _randn(3 * H, seed=194)
    lw, lb = _randn(H, seed=195, mean=1.0), _randn(H, seed=196)
    work = lambda n, smax: (torch.empty(n * nh * H, device=DEV), torch.empty(n * ((smax + L.CHUNK_ROWS - 1) // L.CHUNK_ROWS) * nh * (H + 2), device=DEV),
                            torch.zeros((apl, (n + 63) // 64 * 64, nh * H), dtype=dt, device=DEV))
    ctx, ref = _canary(nseq * H + L.GAP, torch.float32), _canary(nseq * H + L.GAP, torch.float32)

    def fold(s0, n, S_, dst, wk):                                # the uniform entry on n sequences of S_ rows from sequence s0
        u, part, z = wk
        _lib.check(lib.vtq_k_cls_fold(q.data_ptr() + s0 * H * 4, Wp.data_ptr(), 3 * H * H, bqkv.data_ptr(), x.data_ptr() + int(row0[s0]) * H * 4, S_ * H,
                                      lw.data_ptr(), lb.data_ptr(), n, S_, H, num_code(fmt), 0, u.data_ptr(), part.data_ptr(), z.data_ptr(),
                                      z.shape[1] * nh * H, dst.data_ptr() + s0 * H * 4, stream()))
    big = work(nseq, max(lengths))
    seqs = _checked_sequences(case, fmt, row0, rows)
    if "lengths" in case.dims:
        arr = (C.c_int32 * nseq)(*lengths)
        u, part, z = big
        _lib.check(lib.vtq_vl_cls_fold(q.data_ptr(), Wp.data_ptr(), 3 * H * H, bqkv.data_ptr(), x.data_ptr(), lw.data_ptr(), lb.data_ptr(), nseq, arr, H,
                                       num_code(fmt), 0, u.data_ptr(), part.data_ptr(), z.data_ptr(), z.shape[1] * nh * H, ctx.data_ptr(), stream()))
        assert len(seqs) >= 64
        small = work(1, max(lengths))
        for j in seqs:                                           # the sequence alone: the entry's own contract
            fold(j, 1, lengths[j], ref, small)
        torch.cuda.synchronize()
        for j in seqs:
            assert torch.equal(_bits(ctx[j * H:(j + 1) * H]), _bits(ref[j * H:(j + 1) * H])), f"sequence {j}"
        assert bool((_bits(ctx[:nseq * H]) != CANARY32).all()), "an output was never stored"
    else:
        fold(0, nseq, S, ctx, big)
        small = work(L.SLICE_SEQS, S)
        for s0 in range(0, nseq, L.SLICE_SEQS):
            fold(s0, min(L.SLICE_SEQS, nseq - s0), S, ref, small)
        _same(ctx, ref, "ctx")
    _kept(ctx[nseq * H:], "behind ctx")
    W64 = planes_value(Wp)
    err = mx = 0.0
    for j in seqs:
        want = _fold_fp64(x, q[j], W64, bqkv, lw, lb, int(row0[j]), lengths[j], H)
        err, mx = max(err, (ctx[j * H:(j + 1) * H].double() - want).abs().max().item()), max(mx, want.abs().max().item())
    print(f"[{name} {fmt}] fp64 error {err / mx:.3g} (bound {ATTN_TOL[fmt]})")
    assert err / mx < ATTN_TOL[fmt], err / mx
    _leave(case, fmt)


@pytest.mark.parametrize("fmt", L.CASES["cls_fold"].fmts)
def test_cls_fold(fmt, mem):
    """5582 sequences of 501 fp32 rows: x passes 2^30 floats in sequence 2790 and 2^31 floats in the last one."""
    _cls_fold("cls_fold", fmt)


@pytest.mark.parametrize("fmt", L.CASES["cls_fold_varlen"].fmts)
def test_cls_fold_varlen(fmt, mem):
    _cls_fold("cls_fold_varlen", fmt)


# ---- the uniform image path: vtq_k_image_normalize, vtq_k_avgpool2, vtq_k_gather_patches -----------------------------------------
def test_images_uniform(mem):
    """11 images of 8192 x 8192: the fp32 level-0 planes pass 2^31 floats in the last image (the bytes of the uint8 input 2^31 in it too),
    and so does what vtq_k_avgpool2 and vtq_k_gather_patches read.  Reference 1: every image alone."""
    case = L.CASES["images_uniform"]
    lib = _enter(case, "")
    NI, side, N, P = case.count, case.dims["side"], case.dims["N"], case.dims["P"]
    half, px = side // 2, side * side
    img, g = torch.empty((NI, side, side, 3), dtype=torch.uint8, device=DEV), _gen(201)
    for i in range(NI):
        img[i].random_(0, 256, generator=g)
    flips = torch.randint(0, 2, (NI, 2), generator=_gen(202), device=DEV, dtype=I32)
    flips[NI - 1] = 1
    fl = flips.cpu().tolist()
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    lv0, lv1 = _canary(NI * 3 * px + L.GAP, torch.float32), _canary(NI * 3 * half * half + L.GAP, torch.float32)
    _lib.check(lib.vtq_k_image_normalize(img.data_ptr(), lv0.data_ptr(), NI, side, side, flips.data_ptr(), mean, std, stream()))
    _lib.check(lib.vtq_k_avgpool2(lv0.data_ptr(), lv1.data_ptr(), NI * 3, side, side, stream()))
    ref0, ref1 = torch.empty(3 * px, device=DEV), torch.empty(3 * half * half, device=DEV)
    for i in range(NI):
        _refill(ref0), _refill(ref1)
        _lib.check(lib.vtq_k_image_normalize(img.data_ptr() + i * px * 3, ref0.data_ptr(), 1, side, side, flips.data_ptr() + i * 8, mean, std, stream()))
        _lib.check(lib.vtq_k_avgpool2(lv0.data_ptr() + i * 3 * px * 4, ref1.data_ptr(), 3, side, side, stream()))
        _same(lv0[i * 3 * px:(i + 1) * 3 * px], ref0, f"level 0 of image {i}")
        _same(lv1[i * 3 * half * half:(i + 1) * 3 * half * half], ref1, f"level 1 of image {i}")
    _kept(lv0[NI * 3 * px:], "behind level 0"), _kept(lv1[NI * 3 * half * half:], "behind level 1")
    # fp64 on rows of the level planes: (image, channel, y)
    t0, t1 = lv0[:NI * 3 * px].view(NI, 3, side, side), lv1[:NI * 3 * half * half].view(NI, 3, half, half)
    e0 = e1 = 0.0
    for r in case.check_rows(""):
        ni, c, y = r // (3 * side), (r // side) % 3, r % side
        hf, vf = fl[ni]
        src = img[ni, side - 1 - y if vf else y, :, c].double()
        want = ((src.flip(0) if hf else src) / 255.0 - MEAN[c]) / STD[c]
        e0 = max(e0, (t0[ni, c, y].double() - want).abs().max().item() / want.abs().max().item())
    for r in case.check_rows("", rows=NI * 3 * half):
        ni, c, y = r // (3 * half), (r // half) % 3, r % half
        two = t0[ni, c, 2 * y:2 * y + 2].double().view(2, half, 2)
        want = (two[0, :, 0] + two[0, :, 1] + two[1, :, 0] + two[1, :, 1]) / 4.0
        e1 = max(e1, (t1[ni, c, y].double() - want).abs().max().item() / want.abs().max().item())
    print(f"[images uniform] fp64 error level 0 {e0:.3g}, level 1 {e1:.3g} (bound {RESID_TOL})")
    assert e0 < RESID_TOL and e1 < RESID_TOL, (e0, e1)
    # gather: N patches per image, alternating between the two levels, the last patch of each level in its bottom-right corner
    g = np.random.RandomState(203)
    sid = np.tile(np.arange(N) % 2, (NI, 1)).astype(np.int32)
    dim = np.where(sid == 0, side, half)
    smp = np.stack([g.randint(0, dim - P + 1), g.randint(0, dim - P + 1)], axis=-1).astype(np.int32)
    smp[:, N - 2:] = (dim[:, N - 2:] - P)[..., None]
    samples, sids = torch.from_numpy(smp).to(DEV), torch.from_numpy(sid).to(DEV)
    patches, pos, scales = _canary(NI * N * 3 * P * P + L.GAP, torch.float32), torch.empty(NI, N, 2, device=DEV), torch.empty(NI, N, device=DEV)

    def gather(i0, n, dst):
        ptrs = (C.c_void_p * 2)(lv0.data_ptr() + i0 * 3 * px * 4, lv1.data_ptr() + i0 * 3 * half * half * 4)
        hw = (C.c_int32 * 2)(side, half)
        _lib.check(lib.vtq_k_gather_patches(ptrs, hw, hw, 2, samples.data_ptr() + i0 * N * 8, sids.data_ptr() + i0 * N * 4, dst.data_ptr(),
                                            pos.data_ptr() + i0 * N * 8, scales.data_ptr() + i0 * N * 4, n, N, P, stream()))
    gather(0, NI, patches)
    one = torch.empty(N * 3 * P * P, device=DEV)
    for i in (0, NI - 1):
        _refill(one)
        gather(i, 1, one)
        _same(patches[i * N * 3 * P * P:(i + 1) * N * 3 * P * P], one, f"patches of image {i}")
    _kept(patches[NI * N * 3 * P * P:], "behind patches")
    pv = patches[:NI * N * 3 * P * P].view(NI, N, 3, P, P)
    for ni in range(NI):
        for n in range(N):
            r, c = int(smp[ni, n, 0]), int(smp[ni, n, 1])
            lvl = t0 if sid[ni, n] == 0 else t1
            assert torch.equal(_bits(pv[ni, n]), _bits(lvl[ni, :, r:r + P, c:c + P].contiguous())), (ni, n)
    _leave(case, "")


# ---- the ragged image gathers: vtq_k_gather_patches_u8, vtq_k_gather_patches_planar -----------------------------------------------
def _pyramid64(image, hf, vf, levels):
    """fp64 levels of one normalised CHW image: flips first, then AvgPool2d(2) (an odd last row / column of the FLIPPED image is dropped)."""
    x = image.double()
    x = x.flip(2) if hf else x
    x = x.flip(1) if vf else x
    out = [x]
    for _ in range(levels - 1):
        out.append(torch.nn.functional.avg_pool2d(out[-1][None], 2)[0])
    return out


def _ragged(name, fmt):
    """Three images in one byte buffer of 2^32 bytes and at most a few MiB -- at byte 0, across byte 2^32, wholly behind it -- and only they are filled.
    Patches on every level, flips on.  Reference 1: the same images packed back to back in a small buffer."""
    case = L.CASES[name]
    lib = _enter(case, fmt)
    N, P, levels, sizes = case.dims["N"], case.dims["P"], 3, L.RAGGED_SIZES
    tdt = {"u8": torch.uint8, "fp32": torch.float32, "fp16": torch.float16}[fmt]
    esize = torch.empty((), dtype=tdt).element_size()
    off, total = L.ragged_layout(esize)
    nb = [3 * h * w * esize for h, w in sizes]
    big = torch.empty(total, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    g = _gen(211)
    images = []
    for i, (h, w) in enumerate(sizes):
        v = big[off[i]:off[i] + nb[i]]
        if fmt == "u8":
            v.random_(0, 256, generator=g)
            images.append(((v.view(h, w, 3).permute(2, 0, 1).double() / 255.0) - torch.tensor(MEAN, device=DEV).view(3, 1, 1).double())
                          / torch.tensor(STD, device=DEV).view(3, 1, 1).double())
        else:
            v.view(tdt).uniform_(0.0, 1.0, generator=g)
            images.append((v.view(tdt).view(3, h, w).double() - torch.tensor(MEAN, device=DEV).view(3, 1, 1).double())
                          / torch.tensor(STD, device=DEV).view(3, 1, 1).double())
    small = torch.cat([big[off[i]:off[i] + nb[i]] for i in range(3)])
    flips_host = [(1, 0), (0, 1), (1, 1)]
    rs = np.random.RandomState(212)
    sid = np.tile(np.arange(N) % levels, 3).astype(np.int32)
    smp = np.zeros((3 * N, 2), np.int32)
    for i, (h, w) in enumerate(sizes):
        for n in range(N):
            s = int(sid[i * N + n])
            hh, ww = (h >> s) - P, (w >> s) - P
            smp[i * N + n] = (hh, ww) if n >= N - levels else (rs.randint(0, hh + 1), rs.randint(0, ww + 1))     # the last patch of each level: the corner
    samples, sids = torch.from_numpy(smp).to(DEV), torch.from_numpy(sid).to(DEV)
    flips = torch.tensor(flips_host, dtype=I32, device=DEV)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    T = 3 * N

    def run(buf, offsets):
        t = patches_mod.image_tables(sizes, [N] * 3, esize)
        o = np.asarray(offsets, dtype=np.int64)
        tab = t.tab.copy()
        tab[:, :2] = o.astype("<i8").view("<i4").reshape(-1, 2)
        dev_tab, dev_pi = torch.from_numpy(tab).to(DEV), torch.from_numpy(t.patch_img).to(DEV)
        assert dev_tab.data_ptr() % 16 == 0
        pt, ps, sc = _canary(T * 3 * P * P + L.GAP, torch.float32), _canary(T * 2 + L.GAP, torch.float32), _canary(T + L.GAP, torch.float32)
        as_p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        rest = (dev_tab.data_ptr(), dev_pi.data_ptr(), as_p(o, C.c_int64), as_p(t.H, C.c_int32), as_p(t.W, C.c_int32), as_p(t.row0, C.c_int32), 3,
                samples.data_ptr(), sids.data_ptr(), flips.data_ptr(), mean, std, pt.data_ptr(), ps.data_ptr(), sc.data_ptr(), P, levels, stream())
        if fmt == "u8":
            _lib.check(lib.vtq_k_gather_patches_u8(buf.data_ptr(), buf.numel(), *rest))
        else:
            _lib.check(lib.vtq_k_gather_patches_planar(buf.data_ptr(), buf.numel(), _lib.PIXEL_DTYPES[str(tdt).split(".")[-1]], *rest))
        torch.cuda.synchronize()
        return pt, ps, sc, int(tab[2, 1])
    pt, ps, sc, high = run(big, off)
    assert high == 1                                             # the high offset word of the image behind byte 2^32
    packed = [0, nb[0], nb[0] + nb[1]]
    rpt, rps, rsc, _ = run(small, packed)
    _same(pt, rpt, "patches"), _same(ps, rps, "pos"), _same(sc, rsc, "scales")          # canary tails included
    _kept(pt[T * 3 * P * P:], "behind patches"), _kept(ps[T * 2:], "behind pos"), _kept(sc[T:], "behind scales")
    pv = pt[:T * 3 * P * P].view(T, 3, P, P)
    err = mx = 0.0
    for i in range(3):
        pyr = _pyramid64(images[i], *flips_host[i], levels)
        for n in range(N):
            k = i * N + n
            r, c = int(smp[k, 0]), int(smp[k, 1])
            want = pyr[int(sid[k])][:, r:r + P, c:c + P]
            err, mx = max(err, (pv[k].double() - want).abs().max().item()), max(mx, want.abs().max().item())
    print(f"[{name}] fp64 error {err / mx:.3g} (bound {RESID_TOL})")
    assert err / mx < RESID_TOL, err / mx
    assert torch.equal(sc[:T], sids.float())
    _leave(case, fmt)


def test_images_ragged_u8(mem):
    _ragged("images_ragged_u8", "u8")


@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
def test_images_planar(fmt, mem):
    _ragged(f"images_planar_{fmt}", fmt)


# ---- the engine, through the Python model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", L.CASES["engine"].fmts)
def test_engine_scores_have_the_bits_of_64_pairs_at_a_time(precision, mem):
    """ViT-B/16, one full layer and the CLS tail, 698 pairs of 500 patches = 699 396 token rows in one piece: the `big` planes pass 2^31
    elements in the QKV and fc1 launches (row 699 050 of 3072), the fp32 residual stream 2^31 bytes.  The batch law of
    tests/test_gpu_group.py test_scores_have_the_bits_of_the_pair_alone: the scores are those of the same pairs scored 64 at a time on a
    second model instance.  That runs pack_patches, embed_index, tokens, zero_pad_rows, the embedding GEMM epilogue, rows_ln, the fold and
    final_diff at this size as well."""
    case = L.CASES["engine"]
    _enter(case, precision)
    B, N, step = case.count, case.dims["N"], case.dims["slice_pairs"]
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False), num_rgs=2, num_rcabs=2, ca_reduction=16)
    models = []
    try:
        for _ in range(2):
            m = VTAMIQ(**json.loads(json.dumps(kw)), precision=precision)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 71).items()})
            models.append(m.to(DEV).eval())
        assert models[0].spec.num_tokens == 1 and models[0].spec.hidden_size == case.dims["H"]
        g = _gen(221)
        pr = torch.empty(B, N, 3, 16, 16, device=DEV).uniform_(-1.0, 1.0, generator=g)
        pd = torch.empty(B, N, 3, 16, 16, device=DEV).uniform_(-1.0, 1.0, generator=g)
        qr = torch.empty(B, N, 2, device=DEV).uniform_(0.0, 1.0, generator=g).clamp_(max=1.0 - 1e-6)
        qd = torch.empty(B, N, 2, device=DEV).uniform_(0.0, 1.0, generator=g).clamp_(max=1.0 - 1e-6)
        with torch.no_grad():
            q = models[0]((pr, pd), (qr, qd), (None, None))[0]
            assert models[0]._read_flags() == 0                  # vtq_input_errors (a set bit would already have raised in forward)
            ref = torch.cat([models[1]((pr[i:i + step], pd[i:i + step]), (qr[i:i + step], qd[i:i + step]), (None, None))[0] for i in range(0, B, step)])
            assert models[1]._read_flags() == 0
        torch.cuda.synchronize()
        assert q.shape == (B,) and bool(torch.isfinite(q).all()) and float(q.std()) > 0
        differ = (_bits(q) != _bits(ref)).nonzero().view(-1)
        assert differ.numel() == 0, f"{differ.numel()} of {B} scores differ from 64 pairs at a time, first pair {int(differ[0])}"
    finally:
        for m in models:
            m._release_engine()
    _leave(case, precision)
