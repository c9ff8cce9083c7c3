"""Where every kernel entry of include/vtamiq_hip.h reads and writes, pinned with guard bands (tests/footprint.py has the method and its limits).

Every buffer handed to an entry is carved from one arena: guards around it, holes inside it (pitch gaps, plane gaps, rows the contract says
are not stored), and "value irrelevant" bytes where the header lets a kernel load without using the value.  Arena.run_twice launches with
all of these filled with 0x00 and again with 0xFF: no guard or hole may change, and the owned outputs of the two runs must be bit-identical;
the outputs are then compared with the fp64 references and tolerances of tests/test_gpu_kernels.py, tests/test_gpu_cls_fold.py,
tests/test_gpu_forward_vit.py and tests/test_validation_metrics.py (imported, none new), so the identity is not vacuous.

CONTRACTS is the table the tests implement, one line per pointer argument, taken from the header (which states the same in words a caller
can allocate from).  The operands of vtq_k_attention and vtq_k_skinny_linear get EXACTLY the promised extent: the loads the header allows
behind the last sequence / the last row land in "value irrelevant" rows, anything further would be a guard whose value shows in an output.
"""

import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests.footprint import Arena, FootprintError
from tests.gpu_util import FORMATS, elt_dtype, num_code, planes_of, planes_value, stream, to_planes
from tests.test_gpu_cls_fold import LOG2_SCALE, Case as FoldCase, _err as fold_err
from tests.test_gpu_forward_vit import PROBS_TOL
from tests.test_gpu_kernels import ATTN_TOL, FMTS, HEAD_TOL, LN_TOL, OUT_TOL, RESID_TOL, SKINNY_TOL, _attention_ref, _randn
from tests.test_validation_metrics import TOL as METRIC_TOL
from vtamiq_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


def _up(a, b):
    return (a + b - 1) // b * b


def attention_overread_rows(S_pad):
    """Rows behind nseq * S_pad that vtq_k_attention may load, from the code: the 4-wave kernel loads Q for every lane of its 128-row query
    blocks unconditionally (csrc/attention.hip, `qf[pl][t] = ...` of attention_kernel), so the last sequence's last block reaches row
    ceil128(S_pad) - 1 of that sequence; K / V tiles of 64 keys reach ceil64(S) - 1 <= that; the 8-wave kernel clamps its Q rows to the
    sequence and reaches the K / V figure only.  At most 127 (S_pad % 128 == 1)."""
    return _up(S_pad, 128) - S_pad


# entry -> {argument: what the entry may read (R) / write (W) through it}; everything else around the buffer is guard.
CONTRACTS = {
    "vtq_k_split": {
        "src": "R numel fp32",
        "dst": "W planes x numel 16-bit at dst + p * plane_stride; [numel, plane_stride) untouched"},
    "vtq_k_layernorm": {
        "x": "R rows x H fp32", "w, b": "R H fp32",
        "out": "W planes x [rows][H] 16-bit, o_plane apart; [rows * H, o_plane) untouched"},
    "vtq_k_gemm": {
        "A": "R activation planes x [M][lda], columns [0, K) only, a_plane apart", "W": "R weight planes x [N][K]", "bias": "R N fp32",
        "gamma": "R N fp32 (epilogue 2, may be NULL)", "x_f32": "R/W [M][N] fp32 (epilogue 2 only)",
        "out16": "W activation planes x [M][ldo], columns [0, N) only, o_plane apart (epilogues 0, 1 only)"},
    "vtq_k_gemm_rowln": {
        "A": "R 2 planes x [M][lda], columns [0, K)", "W": "R 2 planes x [768][K]", "bias, gamma, ln_w, ln_b": "R 768 fp32",
        "x_f32": "R/W rows [0, M) of [*][768] fp32", "out16": "W rows [0, M) of 2 planes x [*][768], o_plane apart (ln_w != NULL only)"},
    "vtq_k_attention": {
        "qkv": "R planes x rows [0, (nseq - 1) * S_pad + ceil128(S_pad)) of [*][3H]: at most 127 rows behind nseq * S_pad, whose values (and "
               "those of rows [S, S_pad) as keys) reach no output row",
        "out": "W planes x rows [0, nseq * S_pad) of [*][H] -- rows [S, S_pad) of a sequence included (the attention of the pad rows' own "
               "queries over the keys < S) -- nothing at or behind row nseq * S_pad"},
    "vtq_k_attention_probs": {
        "qkv": "R planes x rows [s * S_pad, s * S_pad + S) of sequence s, columns [0, 2H)", "probs": "W nseq * (H / 64) * S * S fp32"},
    "vtq_k_skinny_linear": {
        "xa": "R planes x rows [0, ceil64(R)) of [*][ldx], columns [0, K); rows >= R reach no output",
        "W": "R planes x rows [0, ceil16(N)) of [*][K]; rows >= N reach no output", "bias": "R N fp32",
        "res, aux": "R rows [0, R) x columns [0, N) of [*][ldr] fp32 (epilogues 3, 4)", "post_slope, next_slope, gamma": "R 1 / 1 / N fp32",
        "y": "W rows [0, R) x columns [0, ycols) of [*][ldy] fp32",
        "ya": "W planes x rows [0, R) x columns [0, ceil4(N - pcol0)) of [*][ldya] (columns >= N - pcol0: zeros), ya_plane apart"},
    "vtq_k_cls_fold": {
        "q": "R nseq x H fp32", "wqkv": "R planes x rows [H, 3H) of [3H][H]", "bqkv": "R [2H, 3H) fp32", "ln_w, ln_b": "R H fp32",
        "x": "R rows [0, S) of each sequence at x + r * seq_stride; [S * H, seq_stride) never used",
        "u": "W/R nseq * (H/64) * H fp32", "part": "W/R nseq * ceil(S / chunk_rows) * (H/64) * (H + 2) fp32",
        "z": "W rows [0, nseq), R rows [0, ceil64(nseq)) of planes x [*][(H/64) * H]; rows >= nseq reach no output", "ctx": "W nseq x H fp32"},
    "vtq_vl_cls_fold": {
        "q, wqkv, bqkv, ln_w, ln_b": "as vtq_k_cls_fold", "seq_len": "HOST nseq int32",
        "x": "R rows [0, sum of the lengths), packed; sequence j reads rows [row0[j], row0[j] + seq_len[j]) only",
        "u": "W/R nseq * (H/64) * H fp32",
        "part": "W/R nseq * ceil(max length / chunk_rows) * (H/64) * (H + 2) fp32; a sequence's slots behind its own chunks untouched",
        "z": "as vtq_k_cls_fold", "ctx": "W nseq x H fp32"},
    "vtq_k_diffnet_head": {"d": "R HB x H fp32", "q_out": "W HB fp32"},
    "vtq_k_image_normalize": {"images": "R NI*H*W*3 uint8", "flips": "R NI x 2 int32 (may be NULL)", "out": "W NI*3*H*W fp32"},
    "vtq_k_avgpool2": {"in": "R NC*H*W fp32", "out": "W NC*(H/2)*(W/2) fp32"},
    "vtq_k_gather_patches": {
        "levels[l]": "R NI*3*hs[l]*ws[l] fp32", "samples": "R NI*N*2 int32", "scale_ids": "R NI*N int32 (may be NULL)",
        "patches": "W NI*N*3*P*P fp32", "pos": "W NI*N*2 fp32", "scales": "W NI*N fp32 (may be NULL)"},
    "vtq_k_repeat_mean": {"q": "R R*N fp32", "out": "W N fp64"},
    "vtq_k_rank_metrics": {"a, b": "R N fp64", "work": "W/R 4N fp64", "counts": "W 3 int64", "out": "W 3 fp64"},
}
HOST_ONLY = {"vtq_k_gemm_tile_rule", "vtq_k_attention_rule", "vtq_k_gemm_schedule", "vtq_k_cls_fold_chunk_rows", "vtq_vl_attention_blocks"}
PINNED_ELSEWHERE = {"vtq_vl_attention": "tests/test_gpu_varlen.py (the same arena, beside vtq_forward_varlen)"}


def print_contracts():
    print("pinned footprint contract per entry (tests/test_gpu_footprint.py CONTRACTS)")
    for entry, args in CONTRACTS.items():
        for i, (arg, what) in enumerate(args.items()):
            print(f"  {entry if i == 0 else '':24s} {arg:32s} {what}")
    print("attention over-read behind nseq * S_pad, derived from csrc/attention.hip: ceil128(S_pad) - S_pad rows (4-wave Q loads), "
          "ceil64(S) - S_pad (K / V tiles, both kernels); maximum over S_pad:", max(attention_overread_rows(s) for s in range(1, 1025)))


def test_contract_table_covers_every_kernel_entry():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vtamiq_hip.h")).read()
    entries = set(re.findall(r"\b(vtq_(?:k|vl)_\w+)\s*\(", hdr)) - HOST_ONLY - set(PINNED_ELSEWHERE)
    assert entries == set(CONTRACTS), entries ^ set(CONTRACTS)
    assert max(attention_overread_rows(s) for s in range(1, 2049)) == 127
    print_contracts()


# ---- layout helper ------------------------------------------------------------------------------------------------------
class Layout:
    """Collect the buffers of one call, then build an arena of exactly the size they need."""

    def __init__(self):
        self.specs, self.post = [], []

    def add(self, name, shape, dtype, pitch=None, plane=None):
        self.specs.append((name, tuple(shape), dtype, pitch, plane))

    def planes(self, name, npl, rows, cols, ld, plane, dtype, alloc_rows=None):
        """npl planes of [alloc_rows or rows][ld] elements, `plane` elements apart; columns [cols, ld), rows [rows, alloc_rows) and the
        space between planes are holes.  v[name + '.v'] is the owned [npl][rows][cols] view."""
        isz = torch.empty((), dtype=dtype).element_size()
        ar = alloc_rows or rows
        assert plane >= ar * ld or npl == 1
        self.add(name, ((npl - 1) * plane + ar * ld,), dtype, ld * isz, plane * isz)

        def post(a, v):
            for pl in range(npl):
                if ld > cols:
                    a.hole(name, f"columns [{cols}, {ld}) of plane {pl}", (pl * plane + cols) * isz, (ld - cols) * isz, ld * isz, rows)
                if ar > rows:
                    a.hole(name, f"rows [{rows}, {ar}) of plane {pl}", (pl * plane + rows * ld) * isz, (ar - rows) * ld * isz)
                if pl + 1 < npl and plane > ar * ld:
                    a.hole(name, f"gap behind plane {pl}", (pl * plane + ar * ld) * isz, (plane - ar * ld) * isz)
            v[name + ".v"] = v[name].as_strided((npl, rows, cols), (plane, ld, 1))
        self.post.append(post)

    def build(self):
        a = Arena(fp.arena_bytes([(s[1], s[2], s[3]) for s in self.specs]), DEV)
        v = {name: a.carve(name, shape, dtype, pitch, plane) for name, shape, dtype, pitch, plane in self.specs}
        for p in self.post:
            p(a, v)
        return a, v


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


# ---- the check can fail -------------------------------------------------------------------------------------------------
def test_a_store_into_a_guard_is_reported():
    """A torch indexed store of one element lands where a mis-addressed kernel store would: named by buffer, side and offset."""
    L = Layout()
    L.add("x", (16, 64), F32)
    L.planes("out", 2, 8, 24, 32, 8 * 32 + 16, torch.float16)
    a, v = L.build()
    a.fill_guards(0x00)
    assert a.violations(0x00) == []
    behind = v["x"].as_strided((17, 64), (64, 1))               # one row more than the buffer has
    behind[16, 5] = 1.0
    v["out"][3 * 32 + 30] = 1.0                                  # a gap column of plane 0
    got = {(r.buffer, r.side): r for r in a.violations(0x00)}
    assert set(got) == {("x", "after"), ("out", "hole:columns [24, 32) of plane 0")}
    r = got[("x", "after")]
    assert r.offset == 5 * 4 + 2 and r.changed == 2 and r.where == "row 16 column 5"       # 1.0f = 00 00 80 3F: two bytes differ from 0x00
    assert got[("out", "hole:columns [24, 32) of plane 0")].where == "plane 0 row 3 column 30"
    a.fill_guards(0xFF)
    assert a.violations(0xFF) == []


@pytest.mark.parametrize("short", [True, False])
def test_an_operand_carved_one_row_short_fails_bit_identity_for_that_row(short):
    """vtq_k_gemm with an A view one row short: its last row lies in the guard (still inside the arena), so the two fills give different
    bits in exactly the last output row -- and with the whole operand the same call passes."""
    lib = _lib.load()
    fmt, M, N, K = "fp16", 256, 256, 128
    A, W, bias = _randn(M, K, seed=2), _randn(N, K, seed=3, scale=0.05), _randn(N, seed=4)
    Ap, Wp = to_planes(A, fmt, "a"), to_planes(W, fmt, "w")
    L = Layout()
    L.add("A", (M - 1 if short else M, K), torch.float16)
    L.add("W", (N, K), torch.float16)
    L.add("bias", (N,), F32)
    L.add("out", (M, N), torch.float16)
    a, v = L.build()
    v["A"].copy_(Ap[0, : v["A"].shape[0]])
    v["W"].copy_(Wp[0])
    v["bias"].copy_(bias)

    def launch():
        _lib.check(lib.vtq_k_gemm(v["A"].data_ptr(), M * K, K, v["W"].data_ptr(), N * K, M, N, K, num_code(fmt), 0, v["bias"].data_ptr(), None,
                                  None, v["out"].data_ptr(), M * N, N, stream()))
    if short:
        with pytest.raises(FootprintError) as e:
            a.run_twice(launch, lambda: [v["out"]])
        assert not e.value.violations and list(e.value.mismatch) == [0]
        rows = e.value.mismatch[0].any(-1).nonzero().flatten().tolist()
        assert rows == [M - 1], rows
    else:
        (got,) = a.run_twice(launch, lambda: [v["out"]])
        ref = planes_value(Ap) @ planes_value(Wp).t() + bias.double()
        assert _rel(got, ref) < OUT_TOL[fmt]


# ---- vtq_k_split, vtq_k_layernorm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("numel", [4, 1024, 1028])
def test_split(numel, planes, f16):
    """numel: the smallest legal one, one 256-thread block of 4-element vectors, one vector past it.  Bit-exact against the definition."""
    lib = _lib.load()
    dt = torch.float16 if f16 else torch.bfloat16
    ps = numel + 24
    x = _randn(numel, seed=numel)
    x[:4] = torch.tensor([1e-6, -3e-7, 6.1e-5, 65000.0 if f16 else 1e30])
    L = Layout()
    L.add("src", (numel,), F32)
    L.planes("dst", planes, 1, numel, numel, ps, dt)
    a, v = L.build()
    v["src"].copy_(x)
    (got,) = a.run_twice(lambda: _lib.check(lib.vtq_k_split(v["src"].data_ptr(), v["dst"].data_ptr(), ps, numel, f16, planes, stream())),
                         lambda: [v["dst.v"]], prepare=lambda: v["dst.v"].zero_())
    hi = x.to(dt)
    assert torch.equal(got[0, 0], hi)
    if planes == 2:
        assert torch.equal(got[1, 0], (x - hi.float()).to(dt))


@pytest.mark.parametrize("fmt", ["bf16", "bf16x3", "fp16", "fp16x3"])
@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("rows", [1, 515])
def test_layernorm(rows, H, fmt):
    lib = _lib.load()
    npl = planes_of(fmt, "a")
    o_plane = rows * H + 64
    x = _randn(rows, H, seed=13, scale=3.0) + 0.7
    w, b = _randn(H, seed=14) + 1.0, _randn(H, seed=15)
    L = Layout()
    L.add("x", (rows, H), F32)
    L.add("w", (H,), F32)
    L.add("b", (H,), F32)
    L.planes("out", npl, rows, H, H, o_plane, elt_dtype(fmt))
    a, v = L.build()
    v["x"].copy_(x), v["w"].copy_(w), v["b"].copy_(b)
    (got,) = a.run_twice(lambda: _lib.check(lib.vtq_k_layernorm(v["x"].data_ptr(), v["w"].data_ptr(), v["b"].data_ptr(), v["out"].data_ptr(), o_plane,
                                                                rows, H, FORMATS[fmt][0], npl, stream())),
                         lambda: [v["out.v"]], prepare=lambda: v["out.v"].zero_())
    ref = torch.nn.functional.layer_norm(x.double(), (H,), w.double(), b.double(), 1e-6)
    assert _rel(planes_value(got), ref) < LN_TOL[fmt]


# ---- vtq_k_gemm ---------------------------------------------------------------------------------------------------------
def _gemm_case(fmt, M, N, K, pitched, epis, variants, sample=None):
    lib = _lib.load()
    dt, apl, wpl = elt_dtype(fmt), planes_of(fmt, "a"), planes_of(fmt, "w")
    lda, ldo = (K + 16, N + 64) if pitched else (K, N)
    a_plane, o_plane = (M * lda + 48, M * ldo + 80) if pitched else (M * lda, M * ldo)
    A, W, bias, gamma = _randn(M, K, seed=2), _randn(N, K, seed=3, scale=0.05), _randn(N, seed=4), _randn(N, seed=11)
    x0 = _randn(M, N, seed=12)
    Ap, Wp = to_planes(A, fmt, "a"), to_planes(W, fmt, "w")
    L = Layout()
    L.planes("A", apl, M, K, lda, a_plane, dt)
    L.planes("W", wpl, N, K, K, N * K, dt)
    L.add("bias", (N,), F32)
    L.add("gamma", (N,), F32)
    L.add("x", (M, N), F32)
    L.planes("out", apl, M, N, ldo, o_plane, dt)
    a, v = L.build()
    v["A.v"].copy_(Ap), v["W.v"].copy_(Wp), v["bias"].copy_(bias), v["gamma"].copy_(gamma)
    rows = torch.arange(M, device=DEV) if sample is None else sample.to(DEV)
    pre = planes_value(Ap)[rows] @ planes_value(Wp).t() + bias.double()
    ref = {0: pre, 1: torch.nn.functional.gelu(pre), 2: x0[rows].double() + gamma.double() * pre}
    try:
        for epi in epis:
            for variant in variants:
                _lib.check(lib.vtq_debug_gemm_variant(variant))
                res = epi == 2

                def launch():
                    _lib.check(lib.vtq_k_gemm(v["A"].data_ptr(), a_plane, lda, v["W"].data_ptr(), N * K, M, N, K, num_code(fmt), epi, v["bias"].data_ptr(),
                                              v["gamma"].data_ptr() if res else None, v["x"].data_ptr() if res else None,
                                              None if res else v["out"].data_ptr(), o_plane, ldo, stream()))

                def prepare():
                    v["x"].copy_(x0)
                    v["out.v"].zero_()
                try:
                    (got,) = a.run_twice(launch, lambda: [v["x"] if res else v["out.v"]], prepare=prepare)
                except FootprintError as e:
                    raise AssertionError(f"{fmt} M={M} N={N} K={K} epilogue {epi} tile variant {variant}: {e}") from e
                if res:
                    assert not bool(v["out.v"].float().any()), "epilogue 2 wrote out16"
                    err, tol = _rel(got[rows], ref[2]), RESID_TOL
                else:
                    assert torch.equal(v["x"], x0), f"epilogue {epi} wrote x_f32"
                    err, tol = _rel(planes_value(got)[rows], ref[epi]), OUT_TOL[fmt]
                assert err < tol, (fmt, epi, variant, err)
    finally:
        _lib.check(lib.vtq_debug_gemm_variant(-1))


@pytest.mark.parametrize("fmt", FMTS)
def test_gemm_one_tile_smallest_k(fmt):
    """(256, 256, smallest legal K): one 256x256 tile, four 128x128, sixteen 64x64; every epilogue and tile shape."""
    _gemm_case(fmt, 256, 256, 128 if FORMATS[fmt][1] == 1 else 64, False, (0, 1, 2), (-1, 0, 1, 2, 3))


@pytest.mark.parametrize("fmt", FMTS)
def test_gemm_honours_pitches_and_plane_strides(fmt):
    """lda = K + 16, ldo = N + 64, a_plane > M * lda, o_plane > M * ldo: the gap columns and the space between planes are holes -- a load
    or store that ignores a pitch or takes M * N for the plane stride shows."""
    _gemm_case(fmt, 512, 768, 768, True, (0, 1, 2), (-1, 0, 1, 2, 3))


@pytest.mark.parametrize("fmt", ["bf16", "fp16x2", "fp16x3"])
def test_gemm_many_tiles_per_workgroup(fmt):
    """270 tiles: every workgroup of the persistent launch walks several, half tiles close the lists; one format per term count."""
    M = 256 * 30
    sample = torch.cat([torch.arange(0, M, 97), torch.tensor([127, 128, 255, 256, M - 129, M - 128, M - 1])])
    _gemm_case(fmt, M, 2304, 768, False, (0,), (0,), sample=sample)


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
@pytest.mark.parametrize("use_ln", [True, False])
@pytest.mark.parametrize("M,K", [(128, 128), (128, 768), (384, 128), (384, 768)])
def test_gemm_rowln(M, K, use_ln, fmt):
    """M rows inside buffers of round_up(M, 256) rows: rows >= M of x_f32 and of the LayerNorm planes are holes; lda > K."""
    lib = _lib.load()
    N, dt = 768, elt_dtype(fmt)
    Mp, lda = _up(M, 256), K + 16
    a_plane, o_plane = M * lda + 32, Mp * N
    A, W, bias, gamma = _randn(M, K, seed=21), _randn(N, K, seed=22, scale=0.03), _randn(N, seed=23), _randn(N, seed=24) + 1.0
    lw, lb, x0 = _randn(N, seed=25) + 1.0, _randn(N, seed=26), _randn(M, N, seed=27, scale=2.0)
    Ap, Wp = to_planes(A, fmt, "a"), to_planes(W, fmt, "w")
    L = Layout()
    L.planes("A", 2, M, K, lda, a_plane, dt)
    L.planes("W", 2, N, K, K, N * K, dt)
    for n in ("bias", "gamma", "lw", "lb"):
        L.add(n, (N,), F32)
    L.planes("x", 1, M, N, N, Mp * N, F32, alloc_rows=Mp)
    L.planes("out", 2, M, N, N, o_plane, dt, alloc_rows=Mp)
    a, v = L.build()
    v["A.v"].copy_(Ap), v["W.v"].copy_(Wp), v["bias"].copy_(bias), v["gamma"].copy_(gamma), v["lw"].copy_(lw), v["lb"].copy_(lb)

    def launch():
        _lib.check(lib.vtq_k_gemm_rowln(v["A"].data_ptr(), a_plane, lda, v["W"].data_ptr(), N * K, M, K, num_code(fmt), v["bias"].data_ptr(),
                                        v["gamma"].data_ptr(), v["x"].data_ptr(), _ptr(v["lw"]) if use_ln else None, _ptr(v["lb"]) if use_ln else None,
                                        _ptr(v["out"]) if use_ln else None, o_plane, stream()))

    def prepare():
        v["x.v"][0].copy_(x0)
        v["out.v"].fill_(7.0)
    x, out = a.run_twice(launch, lambda: [v["x.v"][0], v["out.v"]], prepare=prepare)
    ref = x0.double() + gamma.double() * (planes_value(Ap) @ planes_value(Wp).t() + bias.double())
    assert _rel(x, ref) < RESID_TOL
    if use_ln:
        ln = torch.nn.functional.layer_norm(x.double(), (N,), lw.double(), lb.double(), 1e-6)      # of the kernel's own fp32 rows
        assert _rel(planes_value(out), ln) < LN_TOL[fmt]
    else:
        assert bool((out == 7.0).all())


# ---- vtq_k_attention, vtq_k_attention_probs -----------------------------------------------------------------------------
ATTN_SHAPES = [(3, 9, 768), (2, 64, 768), (2, 65, 768), (2, 129, 768), (3, 257, 768), (1, 521, 768), (2, 65, 1024)]


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_attention(variant, fmt):
    """qkv has exactly the rows the header promises -- nseq * S_pad + (ceil128(S_pad) - S_pad), the last of them "value irrelevant" -- and
    out exactly nseq * S_pad; packed (S_pad = S) and padded (S_pad = ceil32(S)) pitch.  S = 65, 129, 257, 521: one row past a key tile, a
    4-wave query block, an 8-wave query block; variant 2 on 257 / 521 is the split form."""
    lib = _lib.load()
    dt, npl = elt_dtype(fmt), planes_of(fmt, "a")
    lib.vtq_debug_attention_variant(variant)
    try:
        for nseq, S, H in ATTN_SHAPES:
            for S_pad in (S, _up(S, 32)):
                over = attention_overread_rows(S_pad)
                rows_in, rows_out = nseq * S_pad + over, nseq * S_pad
                qkv = _randn(rows_in, 3 * H, seed=16, scale=1.5)
                qkv[S - 3, H:H + 64] *= 6.0
                P = to_planes(qkv, fmt, "a")
                L = Layout()
                L.add("qkv", (npl, rows_in, 3 * H), dt, 3 * H * 2, rows_in * 3 * H * 2)
                L.add("out", (npl, rows_out, H), dt, H * 2, rows_out * H * 2)
                a, v = L.build()
                v["qkv"].copy_(P)
                a.scratch("qkv", "rows behind the last sequence", rows_out * 3 * H * 2, over * 3 * H * 2, rows_in * 3 * H * 2, npl)
                try:
                    (got,) = a.run_twice(lambda: _lib.check(lib.vtq_k_attention(v["qkv"].data_ptr(), rows_in * 3 * H, v["out"].data_ptr(), rows_out * H,
                                                                                nseq, S, S_pad, H, num_code(fmt), stream())),
                                         lambda: [v["out"]], prepare=lambda: v["out"].zero_())
                except FootprintError as e:
                    raise AssertionError(f"{fmt} variant {variant} nseq={nseq} S={S} S_pad={S_pad} H={H}: {e}") from e
                ref = _attention_ref(planes_value(P)[:rows_out], nseq, S, S_pad, H)
                err = _rel(planes_value(got).view(nseq, S_pad, H)[:, :S], ref)
                assert err < ATTN_TOL[fmt], (fmt, variant, nseq, S, S_pad, H, err)
    finally:
        lib.vtq_debug_attention_variant(-1)


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16", "bf16"])
@pytest.mark.parametrize("nseq,S", [(2, 9), (2, 65), (1, 257)])
def test_attention_probs(nseq, S, fmt):
    """qkv has exactly nseq * S_pad rows ("reads only rows [s * S_pad, s * S_pad + S)"): rows [S, S_pad) of the padded pitch are value
    irrelevant, probs is guarded on both sides."""
    lib = _lib.load()
    H, nh = 768, 12
    dt, npl = elt_dtype(fmt), planes_of(fmt, "a")
    three = FORMATS[fmt][1] == 3
    scale = 0.125 * math.log2(math.e) if three else 1.0
    for S_pad in (S, _up(S, 32)):
        rows = nseq * S_pad
        qkv = _randn(rows, 3 * H, seed=5, scale=0.5)
        qkv[:, :H] *= scale
        P = to_planes(qkv, fmt, "a")
        L = Layout()
        L.add("qkv", (npl, rows, 3 * H), dt, 3 * H * 2, rows * 3 * H * 2)
        L.add("probs", (nseq, nh, S, S), F32)
        a, v = L.build()
        v["qkv"].copy_(P)
        if S_pad > S:
            a.scratch("qkv", "pad rows", S * 3 * H * 2, (S_pad - S) * 3 * H * 2, S_pad * 3 * H * 2, npl * nseq)
        (got,) = a.run_twice(lambda: _lib.check(lib.vtq_k_attention_probs(v["qkv"].data_ptr(), rows * 3 * H, v["probs"].data_ptr(), nseq, S, S_pad, H,
                                                                          num_code(fmt), int(three), stream())),
                             lambda: [v["probs"]], prepare=lambda: v["probs"].zero_())
        val = planes_value(P).view(nseq, S_pad, 3, nh, 64)[:, :S]
        q, k = val[:, :, 0].permute(0, 2, 1, 3) / scale, val[:, :, 1].permute(0, 2, 1, 3)
        ref = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
        assert float((got.double() - ref).abs().max()) <= PROBS_TOL[three]


# ---- vtq_k_skinny_linear ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3", "fp16x2", "fp16", "bf16"])
@pytest.mark.parametrize("R", [1, 5, 64, 65, 130])
def test_skinny_linear(R, fmt):
    """N in {1, 17, 864} x every epilogue: xa has exactly ceil64(R) rows and W exactly ceil16(N) (the rows behind R / N value irrelevant),
    K = 80 zero-padded to 96 in both (owned zeros), ldx > K, ldy > N, ldr > N, ycols < N and pcol0 > 0 where N allows (fp32 columns
    >= ycols, plane rows >= R and the pitch gaps are holes), ldya > N - pcol0."""
    lib = _lib.load()
    dt, apl, wpl = elt_dtype(fmt), planes_of(fmt, "a"), planes_of(fmt, "w")
    K0, K = 80, 96
    Ra, ldx = _up(R, 64), K + 8
    slope, nxt = 0.23, 0.31
    prelu = lambda t, s: torch.where(t >= 0, t, s * t)
    for N in (1, 17, 864):
        Np = _up(N, 16)
        pcol0 = {1: 0, 17: 16, 864: 768}[N]
        ycols = pcol0 or N
        ncol = _up(N - pcol0, 4)                                    # plane columns stored: [N - pcol0, ncol) as zeros
        ldy, ldr, ldya = _up(N, 4) + 8, _up(N, 4) + 4, ncol + 8
        ya_plane = R * ldya + 16
        x, W, bias = _randn(R, K0, seed=20), _randn(N, K0, seed=21, scale=0.05), _randn(N, seed=22)
        res, aux, gamma = _randn(R, N, seed=33), _randn(R, N, seed=34), _randn(N, seed=35)
        xpad = torch.zeros(Ra, K, device=DEV); xpad[:R, :K0] = x
        wpad = torch.zeros(Np, K, device=DEV); wpad[:N, :K0] = W
        xp, wp = to_planes(xpad, fmt, "a"), to_planes(wpad, fmt, "w")
        L = Layout()
        L.planes("xa", apl, Ra, K, ldx, Ra * ldx, dt)
        L.planes("W", wpl, Np, K, K, Np * K, dt)
        L.add("bias", (N,), F32), L.add("gamma", (N,), F32), L.add("slopes", (2,), F32)
        L.planes("res", 1, R, N, ldr, R * ldr, F32)
        L.planes("aux", 1, R, N, ldr, R * ldr, F32)
        L.planes("y", 1, R, ycols, ldy, R * ldy, F32)
        L.planes("ya", apl, R, ncol, ldya, ya_plane, dt)
        a, v = L.build()
        v["xa.v"].copy_(xp), v["W.v"].copy_(wp), v["bias"].copy_(bias), v["gamma"].copy_(gamma), v["slopes"].copy_(torch.tensor([slope, nxt]))
        v["res.v"][0].copy_(res), v["aux.v"][0].copy_(aux)
        if Ra > R:
            a.scratch("xa", "rows >= R", R * ldx * 2, (Ra - R) * ldx * 2, Ra * ldx * 2, apl)       # (their gap columns with them: never read either)
        if Np > N:
            a.scratch("W", "rows >= N", N * K * 2, (Np - N) * K * 2, Np * K * 2, wpl)
        pre = planes_value(xp)[:R] @ planes_value(wp)[:N].t() + bias.double()
        col = torch.arange(N, device=DEV)
        want = {0: pre, 1: torch.nn.functional.gelu(pre), 2: prelu(pre, slope), 3: res.double() + gamma.double() * pre,
                4: res.double() + aux.double() * torch.sigmoid(pre), 5: torch.where(col >= pcol0, torch.relu(pre), pre)}
        for epi in range(6):
            use_next = epi == 3

            def launch():
                _lib.check(lib.vtq_k_skinny_linear(
                    v["xa"].data_ptr(), Ra * ldx, ldx, v["W"].data_ptr(), Np * K, R, N, K, num_code(fmt), epi, v["bias"].data_ptr(),
                    v["slopes"][0:].data_ptr() if epi == 2 else None, v["gamma"].data_ptr() if epi == 3 else None,
                    v["res"].data_ptr() if epi in (3, 4) else None, v["aux"].data_ptr() if epi == 4 else None, ldr, pcol0,
                    v["y"].data_ptr(), ldy, ycols, v["ya"].data_ptr(), ya_plane, ldya, pcol0, v["slopes"][1:].data_ptr() if use_next else None, stream()))

            def prepare():
                v["y.v"].fill_(float("nan"))
                v["ya.v"].fill_(float("nan"))
            try:
                y, ya = a.run_twice(launch, lambda: [v["y.v"][0], v["ya.v"]], prepare=prepare)
            except FootprintError as e:
                raise AssertionError(f"{fmt} R={R} N={N} epilogue {epi}: {e}") from e
            ref = want[epi]
            assert (y.double() - ref[:, :ycols]).abs().max().item() < SKINNY_TOL * max(1.0, ref.abs().max().item()), (fmt, R, N, epi)
            refp = (prelu(ref, nxt) if use_next else ref)[:, pcol0:]
            assert (planes_value(ya)[:, : N - pcol0] - refp).abs().max().item() < OUT_TOL[fmt] * ref.abs().max().item(), (fmt, R, N, epi)
            assert not bool(ya[:, :, N - pcol0:].float().any()), "plane columns >= N are the consumer's zero K-padding"


# ---- vtq_k_cls_fold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16"])
@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("nseq", [1, 3])
def test_cls_fold(nseq, H, fmt):
    """S in {1, chunk, chunk + 1, 131}; seq_stride > S * H (the gap value irrelevant); u, part, z, ctx of exactly the documented sizes (rows
    [nseq, ceil64(nseq)) of z value irrelevant).  Accuracy as tests/test_gpu_cls_fold.py has it: against the un-folded fp64 formula, at most
    twice the error of the full-layer kernels on the same inputs; and the bits of an ordinary call."""
    lib = _lib.load()
    chunk = lib.vtq_k_cls_fold_chunk_rows()
    nh, dt = H // 64, elt_dtype(fmt)
    apl, wpl = planes_of(fmt, "a"), planes_of(fmt, "w")
    Rz = _up(nseq, 64)
    for S in (1, chunk, chunk + 1, 131):
        c = FoldCase(H, nseq, S, fmt, seed=1000 + 7 * S + nseq)
        q = c.query(0)
        stride = S * H + 64
        chunks = (S + chunk - 1) // chunk
        L = Layout()
        L.add("q", (nseq, H), F32)
        L.add("W", (wpl, 3 * H, H), dt, H * 2, 3 * H * H * 2)
        L.add("b", (3 * H,), F32), L.add("lw", (H,), F32), L.add("lb", (H,), F32)
        L.planes("x", nseq, S, H, H, stride, F32)               # "planes" = sequences, seq_stride apart
        L.add("u", (nseq * nh * H,), F32)
        L.add("part", (nseq * chunks * nh * (H + 2),), F32)
        L.add("z", (apl, Rz, nh * H), dt, nh * H * 2, Rz * nh * H * 2)
        L.add("ctx", (nseq, H), F32)
        a, v = L.build()
        v["q"].copy_(q), v["W"].copy_(c.Wp), v["b"].copy_(c.b), v["lw"].copy_(c.lw), v["lb"].copy_(c.lb)
        v["x.v"].copy_(c.x[: nseq * S].view(nseq, S, H))
        a.scratch("z", "rows >= nseq", nseq * nh * H * 2, (Rz - nseq) * nh * H * 2, Rz * nh * H * 2, apl)

        def launch():
            _lib.check(lib.vtq_k_cls_fold(v["q"].data_ptr(), v["W"].data_ptr(), 3 * H * H, v["b"].data_ptr(), v["x"].data_ptr(), stride, v["lw"].data_ptr(),
                                          v["lb"].data_ptr(), nseq, S, H, num_code(fmt), 1 if c.q_log2 else 0, v["u"].data_ptr(), v["part"].data_ptr(),
                                          v["z"].data_ptr(), Rz * nh * H, v["ctx"].data_ptr(), stream()))

        def prepare():
            for n in ("u", "part", "z", "ctx"):
                v[n].zero_()
        try:
            (ctx,) = a.run_twice(launch, lambda: [v["ctx"]], prepare=prepare)
        except FootprintError as e:
            raise AssertionError(f"{fmt} H={H} nseq={nseq} S={S}: {e}") from e
        assert torch.equal(ctx.view(torch.int32), c.fold(q).view(torch.int32)), (fmt, H, nseq, S)
        e_fold = fold_err(ctx, c.ref(q_in=q)[0])
        e_full = fold_err(c.full_layer(0), c.ref(token=0)[0])
        assert e_fold <= 2.0 * e_full, (fmt, H, nseq, S, e_fold, e_full)


# ---- vtq_vl_cls_fold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16x3", "bf16"])
@pytest.mark.parametrize("H", [768, 1024])
def test_vl_cls_fold(H, fmt):
    """Lengths (131, 1, chunk, chunk + 1) and (chunk + 1, 2) packed back to back: x of exactly the sum of the lengths, nothing behind it; u,
    part, z, ctx of exactly the documented sizes, `part` at the pitch of the longest sequence with the slots behind a shorter sequence's own
    chunks holes.  Every sequence has the bits of vtq_k_cls_fold(nseq = 1, S = its length) on its rows, and that entry's accuracy."""
    lib = _lib.load()
    chunk = lib.vtq_k_cls_fold_chunk_rows()
    nh, dt = H // 64, elt_dtype(fmt)
    apl, wpl = planes_of(fmt, "a"), planes_of(fmt, "w")
    for lengths in ((131, 1, chunk, chunk + 1), (chunk + 1, 2)):
        nseq, R, Rz = len(lengths), sum(lengths), 64
        c = FoldCase(H, 1, R, fmt, seed=2000 + R)                   # its x: R rows; the parameters
        starts = [sum(lengths[:j]) for j in range(nseq)]
        ln = c.ln64()[0]
        q = ((ln[starts] @ c.W64[:H].t() + c.b[:H].double()) * (LOG2_SCALE if c.q_log2 else 1.0)).float().contiguous()
        cmax = (max(lengths) + chunk - 1) // chunk
        slot = nh * (H + 2)
        L = Layout()
        L.add("q", (nseq, H), F32)
        L.add("W", (wpl, 3 * H, H), dt, H * 2, 3 * H * H * 2)
        L.add("b", (3 * H,), F32), L.add("lw", (H,), F32), L.add("lb", (H,), F32)
        L.add("x", (R, H), F32)
        L.add("u", (nseq * nh * H,), F32)
        L.add("part", (nseq * cmax * slot,), F32)
        L.add("z", (apl, Rz, nh * H), dt, nh * H * 2, Rz * nh * H * 2)
        L.add("ctx", (nseq, H), F32)
        a, v = L.build()
        v["q"].copy_(q), v["W"].copy_(c.Wp), v["b"].copy_(c.b), v["lw"].copy_(c.lw), v["lb"].copy_(c.lb), v["x"].copy_(c.x[:R])
        a.scratch("z", "rows >= nseq", nseq * nh * H * 2, (Rz - nseq) * nh * H * 2, Rz * nh * H * 2, apl)
        for j, S in enumerate(lengths):
            own = (S + chunk - 1) // chunk
            if own < cmax:
                a.hole("part", f"slots [{own}, {cmax}) of sequence {j}", (j * cmax + own) * slot * 4, (cmax - own) * slot * 4)
        arr = (C.c_int32 * nseq)(*lengths)

        def launch():
            _lib.check(lib.vtq_vl_cls_fold(v["q"].data_ptr(), v["W"].data_ptr(), 3 * H * H, v["b"].data_ptr(), v["x"].data_ptr(), v["lw"].data_ptr(),
                                           v["lb"].data_ptr(), nseq, arr, H, num_code(fmt), 1 if c.q_log2 else 0, v["u"].data_ptr(), v["part"].data_ptr(),
                                           v["z"].data_ptr(), Rz * nh * H, v["ctx"].data_ptr(), stream()))

        def prepare():
            for n in ("u", "part", "z", "ctx"):
                v[n].zero_()
        try:
            (ctx,) = a.run_twice(launch, lambda: [v["ctx"]], prepare=prepare)
        except FootprintError as e:
            raise AssertionError(f"{fmt} H={H} lengths {lengths}: {e}") from e
        for j, (r0, S) in enumerate(zip(starts, lengths)):
            one = FoldCase(H, 1, S, fmt, seed=1)                    # sequence j alone: c's parameters and rows [r0, r0 + S) of its x
            one.Wp, one.W64, one.b, one.lw, one.lb = c.Wp, c.W64, c.b, c.lw, c.lb
            one.x = torch.zeros_like(one.x)
            one.x[:S] = c.x[r0:r0 + S]
            assert torch.equal(ctx[j].view(torch.int32), one.fold(q[j:j + 1])[0].view(torch.int32)), (fmt, H, lengths, j)
            # accuracy as test_cls_fold bounds the uniform entry: the un-folded fp64 formula, twice the full-layer kernels' error
            e_fold = fold_err(ctx[j:j + 1], one.ref(q_in=q[j:j + 1])[0])
            e_full = fold_err(one.full_layer(0), one.ref(token=0)[0])
            assert e_fold <= 2.0 * e_full, (fmt, H, lengths, j, e_fold, e_full)


# ---- vtq_k_diffnet_head -------------------------------------------------------------------------------------------------
def _model(precision="fp16x3", **vit):
    from vtamiq_amd import VTAMIQ, synth
    cfg = dict(variant="ViT-B16", num_keep_layers=2, num_extra_tokens=2, use_layer_scale=True, pretrained=False)
    cfg.update(vit)
    m = VTAMIQ(vit_config=cfg, precision=precision)
    sd = synth.make_state_dict(m.spec, 61)
    m.load_state_dict({k: torch.from_numpy(w) for k, w in sd.items()})
    return m.to(DEV).eval(), sd


@pytest.fixture(scope="module")
def head_model():
    m, sd = _model()
    p = torch.zeros(1, 4, 3, 16, 16, device=DEV)
    with torch.no_grad():
        m((p, p), (torch.zeros(1, 4, 2, device=DEV),) * 2, (None, None))           # creates the engine and loads the weights
    return m, sd


@pytest.mark.parametrize("HB", [1, 5, 65])
def test_diffnet_head(head_model, HB):
    from oracle import vtamiq_oracle as O
    m, sd = head_model
    H = m.spec.hidden_size
    d = _randn(HB, H, seed=62, scale=0.5)
    L = Layout()
    L.add("d", (HB, H), F32)
    L.add("q", (HB,), F32)
    a, v = L.build()
    v["d"].copy_(d)
    (q,) = a.run_twice(lambda: _lib.check(_lib.load().vtq_k_diffnet_head(m._engine, v["d"].data_ptr(), HB, v["q"].data_ptr(), stream())),
                       lambda: [v["q"]], prepare=lambda: v["q"].zero_())
    t = O.to_torch(sd)
    ref = O.q_predictor(t, O.quality_decoder(t, m.spec, d.cpu())).numpy().reshape(-1)
    assert abs(q.cpu().numpy() - ref).max() < HEAD_TOL * max(1.0, abs(ref).max())


# ---- image -> patches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 8])
@pytest.mark.parametrize("NI", [1, 2])
@pytest.mark.parametrize("mode", ["one", "five", "corners"])
def test_image_pyramid_and_gather(mode, NI, P):
    """A 37 x 53 image through three pyramid levels (53, 26, 13 columns: every avgpool drops an odd last row / column), every level and
    output guarded.  Patches at the four corners (row = h - P, col = w - P: the last element of the level is read) of every level that holds
    a P x P patch -- all three for P = 8, the first two for P = 16 -- with scale ids, scales and flips ("corners"); a single last-corner
    patch and five patches of level 0 without them ("one", "five").  Bit-exact against oracle/patch_oracle.py."""
    from oracle import patch_oracle as PO
    lib = _lib.load()
    Hh, Ww = 37, 53
    dims = [(Hh, Ww), (Hh // 2, Ww // 2), (Hh // 4, Ww // 4)]
    rng = np.random.default_rng(7 + NI)
    imgs = rng.integers(0, 256, (NI, Hh, Ww, 3), dtype=np.uint8)
    full = mode == "corners"
    use = [l for l, (h, w) in enumerate(dims) if h >= P and w >= P] if full else [0]
    flips = rng.integers(0, 2, (NI, 2)).astype(np.int32) if full else None
    per_level = []
    for l in use:
        h, w = dims[l]
        pts = [(h - P, w - P)] if mode == "one" else [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)] + ([(3, 5)] if mode == "five" else [])
        per_level.append(np.array(pts, dtype=np.int32).T)                       # (2, n)
    N = sum(p.shape[1] for p in per_level)
    samples = np.broadcast_to(np.concatenate([p.T for p in per_level])[None], (NI, N, 2)).astype(np.int32).copy()
    sids = np.broadcast_to(np.concatenate([np.full(p.shape[1], l) for l, p in zip(use, per_level)])[None], (NI, N)).astype(np.int32).copy()
    L = Layout()
    L.add("img", (NI, Hh, Ww, 3), torch.uint8, Ww * 3)
    L.add("flips", (NI, 2), torch.int32)
    for l, (h, w) in enumerate(dims):
        L.add(f"lv{l}", (NI, 3, h, w), F32)
    L.add("samples", (NI, N, 2), torch.int32), L.add("sids", (NI, N), torch.int32)
    L.add("patches", (NI, N, 3, P, P), F32, P * 4), L.add("pos", (NI, N, 2), F32), L.add("scales", (NI, N), F32)
    a, v = L.build()
    v["img"].copy_(torch.from_numpy(imgs)), v["samples"].copy_(torch.from_numpy(samples)), v["sids"].copy_(torch.from_numpy(sids))
    if full:
        v["flips"].copy_(torch.from_numpy(flips))
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.5, 0.5, 0.5)
    nlv = len(use)
    ptrs = (C.c_void_p * nlv)(*[v[f"lv{l}"].data_ptr() for l in range(nlv)])
    hs, ws = (C.c_int32 * nlv)(*[dims[l][0] for l in range(nlv)]), (C.c_int32 * nlv)(*[dims[l][1] for l in range(nlv)])

    def launch():
        _lib.check(lib.vtq_k_image_normalize(v["img"].data_ptr(), v["lv0"].data_ptr(), NI, Hh, Ww, v["flips"].data_ptr() if full else None, mean, std, stream()))
        for l in (1, 2):
            _lib.check(lib.vtq_k_avgpool2(v[f"lv{l - 1}"].data_ptr(), v[f"lv{l}"].data_ptr(), NI * 3, dims[l - 1][0], dims[l - 1][1], stream()))
        _lib.check(lib.vtq_k_gather_patches(ptrs, hs, ws, nlv, v["samples"].data_ptr(), v["sids"].data_ptr() if full else None, v["patches"].data_ptr(),
                                            v["pos"].data_ptr(), v["scales"].data_ptr() if full else None, NI, N, P, stream()))

    def prepare():
        for n in ("lv0", "lv1", "lv2", "patches", "pos", "scales"):
            v[n].zero_()
    lv0, lv1, lv2, patches, pos, scales = a.run_twice(launch, lambda: [v[n] for n in ("lv0", "lv1", "lv2", "patches", "pos", "scales")], prepare=prepare)
    tens = [PO.transform_img(imgs[k], bool(flips[k, 0]) if full else False, bool(flips[k, 1]) if full else False) for k in range(NI)]
    cur = torch.stack(tens)
    for got in (lv0, lv1, lv2):
        assert torch.equal(got.cpu(), cur)
        cur = torch.nn.functional.avg_pool2d(cur, 2)
    # the oracle walks scales 0 .. len - 1; with P = 16 / one / five only the first levels hold patches
    rp, rq, rs = PO.extract_patches(tens, [[p] * NI for p in per_level], P)
    assert torch.equal(patches.cpu(), rp) and torch.equal(pos.cpu(), rq)
    if full:
        assert torch.equal(scales.cpu(), (rs.float() if rs is not None else torch.zeros(NI, N)))
    else:
        assert not bool(scales.any())                                               # scales == NULL: not written


# ---- validation reductions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1025])
def test_repeat_mean(N, R):
    from oracle import metrics_oracle as MO
    lib = _lib.load()
    q = _randn(R, N, seed=N + R)
    L = Layout()
    L.add("q", (R, N), F32)
    L.add("out", (N,), torch.float64)
    a, v = L.build()
    v["q"].copy_(q)
    (got,) = a.run_twice(lambda: _lib.check(lib.vtq_k_repeat_mean(v["q"].data_ptr(), v["out"].data_ptr(), R, N, stream())), lambda: [v["out"]],
                         prepare=lambda: v["out"].zero_())
    assert np.array_equal(got.cpu().numpy(), MO.average_over_repeats(q.cpu().numpy().reshape(-1), R))      # same summation order: bit-exact


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("N", [2, 255, 256, 257, 1025])
def test_rank_metrics(N, normalize):
    """work[4N], counts[3], out[3] guarded (N = 1 is refused: test_rejected_calls_launch_nothing).  Heavy ties; the statistics oracle/metrics_oracle.py
    computes them from (scipy.stats on normalize_array), the normalised copies and the average-tie ranks exactly."""
    import scipy.stats
    from oracle import metrics_oracle as MO
    lib = _lib.load()
    rng = np.random.default_rng(N)
    an = np.round(rng.uniform(0, 5, N), 1)
    bn = np.round(0.6 * an + rng.standard_normal(N), 1)
    if N == 2:
        an, bn = np.array([1.5, 0.25]), np.array([0.5, 2.0])
    L = Layout()
    L.add("a", (N,), torch.float64), L.add("b", (N,), torch.float64)
    L.add("work", (4 * N,), torch.float64), L.add("counts", (3,), torch.int64), L.add("out", (3,), torch.float64)
    a, v = L.build()
    v["a"].copy_(torch.from_numpy(an)), v["b"].copy_(torch.from_numpy(bn))

    def prepare():
        v["work"].zero_(), v["counts"].zero_(), v["out"].zero_()
    work, counts, out = (t.cpu().numpy() for t in a.run_twice(
        lambda: _lib.check(lib.vtq_k_rank_metrics(v["a"].data_ptr(), v["b"].data_ptr(), N, normalize, v["work"].data_ptr(), v["counts"].data_ptr(),
                                                  v["out"].data_ptr(), stream())), lambda: [v["work"], v["counts"], v["out"]], prepare=prepare))
    aa = MO.normalize_array(an) if normalize else an
    bb = MO.normalize_array(bn) if normalize else bn
    assert np.array_equal(work[:N], aa) and np.array_equal(work[N:2 * N], bb)       # one exactly-rounded subtraction and division each
    assert np.array_equal(work[2 * N:3 * N], scipy.stats.rankdata(aa)) and np.array_equal(work[3 * N:], scipy.stats.rankdata(bb))
    tot = N * (N - 1) // 2
    cd, xt, yt = (int(c) // 2 for c in counts)
    kendall = cd / np.sqrt(tot - xt) / np.sqrt(tot - yt)
    assert abs(kendall - scipy.stats.kendalltau(aa, bb).correlation) <= METRIC_TOL["KROCC"]
    assert abs(out[0] - scipy.stats.spearmanr(aa, bb).correlation) <= METRIC_TOL["SROCC"]
    assert abs(out[1] - scipy.stats.pearsonr(aa, bb)[0]) <= METRIC_TOL["PLCC_NOFIT"]
    assert abs(out[2] - float(np.sqrt(np.mean((aa - bb) ** 2)))) <= METRIC_TOL["RMSE_NOFIT"]


# ---- the forwards: caller-owned tensors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,num_scales", [(1, 8, 0), (3, 45, 3)])
def test_forward_entries_keep_to_the_callers_tensors(B, N, num_scales):
    """vtq_forward (with the token-trace tap), vtq_forward_pairwise and vtq_forward_vit on the engine of a Python model, with every
    CALLER-owned tensor -- patches, pos, scales, the scores, the trace, forward_vit's features / layer states / probabilities -- carved from
    an arena: guards intact, results bit-identical across the two fills and equal to the ordinary call through the model.  The engine's own
    workspace is its own allocation and out of reach of this method (the per-kernel tests above pin the kernels it runs)."""
    from vtamiq_amd import synth
    m, _ = _model(**(dict(num_scales=num_scales) if num_scales else {}))
    spec = m.spec
    Lr, T, H, nh, S = spec.num_layers, spec.num_tokens, spec.hidden_size, spec.num_heads, N + spec.num_tokens
    pa, po, sc = synth.make_inputs(spec, B, N, 22)
    pa2, po2, _ = synth.make_inputs(spec, B, N, 23)
    imgs = [torch.from_numpy(pa[:, 0]), torch.from_numpy(pa[:, 1]), torch.from_numpy(pa2[:, 1])]
    poss = [torch.from_numpy(po[:, 0]), torch.from_numpy(po[:, 1]), torch.from_numpy(po2[:, 1])]
    scl = [torch.from_numpy(sc[:, i % 2]).float() for i in range(3)] if sc is not None else None
    cu = lambda ts: None if ts is None else tuple(t.to(DEV) for t in ts)
    enc = m.transformer.encoder
    enc.return_layers = enc.return_attention = True
    with torch.no_grad():                                                        # the ordinary calls (they also create the engine)
        trace_ref = torch.zeros(Lr + 1, 2 * B, T, H, device=DEV)
        q_ref = m(cu(imgs[:2]), cu(poss[:2]), cu(scl[:2]) if scl else (None, None), _trace=trace_ref)[0]
        q1, q2 = m.forward_pairwise(cu(imgs), cu(poss), cu(scl) if scl else (None,) * 3)
        vit_ref = {}
        for all_tokens in (0, 1):
            x, probs, states = m.forward_vit(imgs[0].to(DEV), poss[0].to(DEV), scl[0].to(DEV) if scl else None, tokens_only=not all_tokens)
            vit_ref[all_tokens] = (x, torch.stack(states), torch.stack(probs))
    torch.cuda.synchronize()
    L = Layout()
    for i in range(3):
        L.add(f"patches{i}", imgs[i].shape, F32, 16 * 4), L.add(f"pos{i}", (B, N, 2), F32), L.add(f"scales{i}", (B, N), F32)
    L.add("q", (B,), F32), L.add("q2", (2 * B,), F32), L.add("trace", (Lr + 1, 2 * B, T, H), F32)
    for at, R in ((0, T), (1, S)):
        L.add(f"vit_x{at}", (B, R, H), F32), L.add(f"vit_states{at}", (Lr, B, R, H), F32), L.add(f"vit_probs{at}", (Lr, B, nh, S, S), F32)
    a, v = L.build()
    for i in range(3):
        v[f"patches{i}"].copy_(imgs[i]), v[f"pos{i}"].copy_(poss[i])
        if scl:
            v[f"scales{i}"].copy_(scl[i])
    lib, eng = m._engine_lib(), m._engine
    p = lambda n: v[n].data_ptr()
    sp = lambda i: p(f"scales{i}") if scl else None
    arr = lambda pre: (C.c_void_p * 3)(*[p(f"{pre}{i}") for i in range(3)])
    outs = ["q", "q2", "trace"] + [f"vit_{n}{at}" for at in (0, 1) for n in ("x", "states", "probs")]

    def launch():
        _lib.check(lib.vtq_set_token_trace(eng, p("trace")))
        try:
            _lib.check(lib.vtq_forward(eng, p("patches0"), p("patches1"), p("pos0"), p("pos1"), sp(0), sp(1), B, N, p("q"), stream()))
        finally:
            lib.vtq_set_token_trace(eng, None)
        _lib.check(lib.vtq_forward_pairwise(eng, arr("patches"), arr("pos"), arr("scales") if scl else None, B, N, p("q2"), stream()))
        for at in (0, 1):
            _lib.check(lib.vtq_forward_vit(eng, p("patches0"), 0, p("pos0"), sp(0), B, N, at, p(f"vit_x{at}"), p(f"vit_states{at}"), p(f"vit_probs{at}"), stream()))

    def prepare():
        for n in outs:
            v[n].zero_()
    got = dict(zip(outs, a.run_twice(launch, lambda: [v[n] for n in outs], prepare=prepare)))
    bits = lambda t: t.contiguous().view(torch.int32)
    assert bool(torch.isfinite(got["q"]).all()) and torch.equal(bits(got["q"]), bits(q_ref))
    assert torch.equal(bits(got["q2"]), bits(torch.cat([q1, q2]))) and torch.equal(bits(got["trace"]), bits(trace_ref))
    for at in (0, 1):
        for n, ref in zip(("x", "states", "probs"), vit_ref[at]):
            assert torch.equal(bits(got[f"vit_{n}{at}"]), bits(ref)), (n, at)
    flags = C.c_int32(-1)
    _lib.check(lib.vtq_input_errors(eng, C.byref(flags), stream()))
    assert flags.value == 0


# ---- rejected calls launch nothing --------------------------------------------------------------------------------------
def test_rejected_calls_launch_nothing():
    """One documented-invalid argument per entry (and the unknown operand format code where an entry takes one): an error comes back and every
    byte of every buffer and guard is as before."""
    lib = _lib.load()
    L = Layout()
    for n in ("in0", "in1", "in2", "out0", "out1", "out2"):
        L.add(n, (1 << 20,), torch.uint8, 4096)
    a, v = L.build()
    a.fill_guards(0xFF)
    g = torch.Generator(device="cpu").manual_seed(1)
    for n in v:
        v[n].copy_(torch.randint(0, 256, (1 << 20,), generator=g, dtype=torch.uint8))
    before = a.mem.clone()
    i0, i1, i2, o0, o1, o2 = (v[n].data_ptr() for n in ("in0", "in1", "in2", "out0", "out1", "out2"))
    s = stream()
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    lv = (C.c_void_p * 5)(i0, i0, i0, i0, i0)
    hw = (C.c_int32 * 5)(32, 32, 32, 32, 32)
    gemm = lambda M=256, N=256, K=128, lda=128, num=17, epi=0: lib.vtq_k_gemm(i0, M * lda, lda, i1, N * K, M, N, K, num, epi, i2, None, None, o0, M * N, N, s)
    skinny = lambda K=64, num=19: lib.vtq_k_skinny_linear(i0, 64 * 64, 64, i1, 16 * 64, 4, 16, K, num, 0, i2, None, None, None, None, 16, 0, o0, 16, 16,
                                                          None, 0, 0, 0, None, s)
    fold = lambda H=768, num=19: lib.vtq_k_cls_fold(i0, i1, 3 * H * H, i2, i0, 2 * H, i2, i2, 1, 2, H, num, 0, o0, o1, o2, 64 * (H // 64) * H, o0, s)
    two = (C.c_int32 * 1)(2)
    vfold = lambda x=i0, nseq=1, seq_len=two, H=768, num=19, q_log2=0: lib.vtq_vl_cls_fold(i0, i1, 3 * H * H, i2, x, i2, i2, nseq, seq_len, H, num, q_log2,
                                                                                       o0, o1, o2, 64 * (H // 64) * H, o0, s)
    calls = {
        "vtq_k_split: numel % 4": lambda: lib.vtq_k_split(i0, o0, 64, 6, 1, 2, s),
        "vtq_k_layernorm: H = 512": lambda: lib.vtq_k_layernorm(i0, i1, i2, o0, 4 * 512, 4, 512, 1, 2, s),
        "vtq_k_gemm: M % 256": lambda: gemm(M=128),
        "vtq_k_gemm: lda % 16": lambda: gemm(lda=136),
        "vtq_k_gemm: N > 4096": lambda: gemm(N=4352),
        "vtq_k_gemm: unknown num": lambda: gemm(num=99),
        "vtq_k_gemm: epilogue 3": lambda: gemm(epi=3),
        "vtq_k_gemm_rowln: M % 128": lambda: lib.vtq_k_gemm_rowln(i0, 64 * 128, 128, i1, 768 * 128, 64, 128, 19, i2, None, o0, i2, i2, o1, 64 * 768, s),
        "vtq_k_gemm_rowln: a 1-term num": lambda: lib.vtq_k_gemm_rowln(i0, 128 * 128, 128, i1, 768 * 128, 128, 128, 17, i2, None, o0, i2, i2, o1, 128 * 768, s),
        "vtq_k_attention: S <= S_pad - 64": lambda: lib.vtq_k_attention(i0, 96 * 2304, o0, 96 * 768, 1, 9, 96, 768, 19, s),
        "vtq_k_attention: unknown num": lambda: lib.vtq_k_attention(i0, 32 * 2304, o0, 32 * 768, 1, 9, 9, 768, 99, s),
        "vtq_k_attention_probs: S_pad < S": lambda: lib.vtq_k_attention_probs(i0, 32 * 2304, o0, 1, 9, 8, 768, 19, 1, s),
        "vtq_k_attention_probs: unknown num": lambda: lib.vtq_k_attention_probs(i0, 32 * 2304, o0, 1, 9, 9, 768, 99, 0, s),
        "vtq_k_skinny_linear: K % 32": lambda: skinny(K=48),
        "vtq_k_skinny_linear: unknown num": lambda: skinny(num=99),
        "vtq_k_cls_fold: H = 512": lambda: fold(H=512),
        "vtq_k_cls_fold: unknown num": lambda: fold(num=99),
        "vtq_vl_cls_fold: NULL x": lambda: vfold(x=None),
        "vtq_vl_cls_fold: NULL seq_len": lambda: vfold(seq_len=None),
        "vtq_vl_cls_fold: nseq = 0": lambda: vfold(nseq=0),
        "vtq_vl_cls_fold: a length of 0": lambda: vfold(nseq=2, seq_len=(C.c_int32 * 2)(2, 0)),
        "vtq_vl_cls_fold: H = 512": lambda: vfold(H=512),
        "vtq_vl_cls_fold: unknown num": lambda: vfold(num=99),
        "vtq_vl_cls_fold: q_log2 on a 1-term num": lambda: vfold(num=17, q_log2=1),
        "vtq_k_diffnet_head: HB = 0": lambda: lib.vtq_k_diffnet_head(None, i0, 0, o0, s),
        "vtq_k_image_normalize: NI = 0": lambda: lib.vtq_k_image_normalize(i0, o0, 0, 8, 8, None, f3, f3, s),
        "vtq_k_avgpool2: H = 1": lambda: lib.vtq_k_avgpool2(i0, o0, 3, 1, 8, s),
        "vtq_k_gather_patches: P = 12": lambda: lib.vtq_k_gather_patches(lv, hw, hw, 1, i1, None, o0, o1, None, 1, 1, 12, s),
        "vtq_k_gather_patches: nlevels = 5": lambda: lib.vtq_k_gather_patches(lv, hw, hw, 5, i1, None, o0, o1, None, 1, 1, 16, s),
        "vtq_k_repeat_mean: R = 0": lambda: lib.vtq_k_repeat_mean(i0, o0, 0, 8, s),
        "vtq_k_rank_metrics: N = 1": lambda: lib.vtq_k_rank_metrics(i0, i1, 1, 1, o0, o1, o2, s),
    }
    assert {k.split(":")[0] for k in calls} == set(CONTRACTS)
    for what, call in calls.items():
        assert call() != 0, what + ": accepted"
        assert lib.vtq_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(a.mem, before)
