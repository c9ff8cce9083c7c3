"""The shapes at which an element index or a byte offset inside ONE buffer passes 2^31 elements, 2^31 bytes or 2^32 bytes (fp32 buffers: 2^30
elements as well), for every kernel entry that takes a row, sequence, element or image count (tests/test_gpu_large_offsets.py), shared the
way tests/helpers.py is -- not a conftest.  Pure Python: tests/test_large_offsets_plan.py checks the arithmetic without a GPU.

The kernels form addresses as (64-bit base of a row, tile or plane) + (32-bit offset bounded by one tile); that is a property of many
separate lines of csrc/*.hip, and a single `int` row-times-pitch product among them would wrap exactly here.  A case states its entry,
every buffer (rows, pitch, element size, planes) and the ONE count it scales with; from those follow the largest element index and byte
offset reached in each buffer, the boundaries crossed, the device bytes, the rows on either side of each crossing, and where a wrapped
index would land instead.

What "crosses" means.  Offsets are counted inside one plane, from the plane's first element -- the product a kernel forms is row * pitch; the
plane stride is a 64-bit argument of every entry -- and over the rows the entry's contract gives a meaning to: slack rows that are only
over-read (the <= 127 rows behind the last sequence of an attention call) do not make a case cross.

Where a wrapped index lands (Buf.wraps).  Four ways to lose the high bits: the byte offset mod 2^32 (a uint32_t byte offset), the element
index mod 2^31 (the sign bit masked off), and the element index or the byte offset as a signed 32-bit value (an `int` product,
sign-extended).  The first two land at a low offset of the same plane: inside the buffer, so such a run does not fault, reads other random data (no compared operand holds
a constant region) or stores into rows that the bitwise comparison covers -- and leaves the canary at the true place.  A signed form whose
low word is in [2^31, 2^32) is negative: for the second plane of a two-plane buffer (plane stride >= 2^31 elements at these shapes) it lands in
the FIRST plane, compared as well; for the first plane it lands in front of the buffer.  Nothing compares that place -- such a store would
fault or hit another allocation -- but the case still fails: the true place keeps its canary (a store) or the output is formed from foreign
data (a load).  test_large_offsets_plan.py asserts exactly this for every crossing, so that no case is vacuous.
"""
from __future__ import annotations

import random
from typing import Callable, NamedTuple

E30, E31, B31, B32 = "2^30 elements", "2^31 elements", "2^31 bytes", "2^32 bytes"
BOUNDARIES = {E30: 1 << 30, E31: 1 << 31, B31: 1 << 31, B32: 1 << 32}      # E*: element index, B*: byte offset; E30 applies to fp32 buffers only
MEM_CAP = 24 << 30                                                        # device bytes one GPU test may hold at its peak
SLICE_ROWS, SLICE_SEQS = 16384, 64                                        # the small launches of the bitwise reference
EVERY = 4097                                                              # every 4097th row goes to the fp64 check
GAP = 4096                                                                # canary elements between the planes and behind the last one


class Buf(NamedTuple):
    """One buffer of a case: `planes` planes of (rows + slack_rows) rows of `pitch` elements of `esize` bytes, `gap` untouched elements behind
    each plane.  role: "in" (read: filled with random data), "out" (written: canary first, compared bit for bit), "io" (both), "ref" (the
    test's own copy for the bitwise reference), "work" (workspace of the entry)."""
    name: str
    rows: int
    pitch: int
    esize: int
    planes: int = 1
    role: str = "in"
    fp32: bool = False
    slack_rows: int = 0
    gap: int = 0

    @property
    def numel(self) -> int:                      # elements of one plane that the entry's contract gives a meaning to
        return self.rows * self.pitch

    @property
    def plane_stride(self) -> int:               # elements from one plane to the next
        return (self.rows + self.slack_rows) * self.pitch + self.gap

    @property
    def alloc_bytes(self) -> int:
        return self.planes * self.plane_stride * self.esize

    @property
    def max_elem(self) -> int:
        return self.numel - 1

    @property
    def max_byte(self) -> int:
        return self.numel * self.esize - 1

    def crossed(self) -> tuple:
        """The boundaries some element of a plane lies AT or BEHIND, in the order of BOUNDARIES."""
        out = []
        if self.fp32 and self.max_elem >= BOUNDARIES[E30]:
            out.append(E30)
        if self.max_elem >= BOUNDARIES[E31]:
            out.append(E31)
        if self.max_byte >= BOUNDARIES[B31]:
            out.append(B31)
        if self.max_byte >= BOUNDARIES[B32]:
            out.append(B32)
        return tuple(out)

    def boundary_elem(self, boundary: str) -> int:
        """The first element index at or behind `boundary`."""
        b = BOUNDARIES[boundary]
        return b if boundary in (E30, E31) else (b + self.esize - 1) // self.esize

    def boundary_rows(self) -> list:
        """The row that holds the first element behind each crossed boundary, and the row in front of it."""
        out = set()
        for b in self.crossed():
            r = self.boundary_elem(b) // self.pitch
            out |= {r - 1, r}
        return sorted(r for r in out if 0 <= r < self.rows)

    def wraps(self, elem: int, plane: int = 0) -> dict:
        """Where element `elem` of plane `plane` lands, as an element index from the BUFFER's base, when its offset loses the high bits."""
        base = plane * self.plane_stride
        s32 = lambda v: (v % (1 << 32)) - ((1 << 32) if (v % (1 << 32)) >> 31 else 0)          # (int32_t)v
        return {"bytes mod 2^32": base + ((elem * self.esize) % (1 << 32)) // self.esize,
                "elements mod 2^31": base + elem % (1 << 31),
                "signed 32-bit": base + s32(elem),
                "signed 32-bit bytes": base + s32(elem * self.esize) // self.esize}


class Case(NamedTuple):
    name: str
    entries: tuple               # the vtq_k_* / vtq_vl_* entries (or the Python model's forward) the GPU test drives
    fmts: tuple                  # operand formats of the GPU test ("" where the entry has none)
    count: int                   # what the shape scales with ...
    gran: int                    # ... and the step of it: one 256-row tile, one 128-row panel, one 4-row workgroup, one sequence, one image
                                 # (0: the ragged image layouts, which are fixed -- ragged_layout -- and checked as layouts)
    unit: str
    target: tuple                # (buffer, boundary) that makes this the case: `count - gran` no longer crosses it
    claims: dict                 # buffer -> the boundaries it crosses
    bufs: Callable               # (count, fmt) -> tuple of Buf
    dims: dict                   # the other extents

    def buffers(self, fmt: str | None = None, count: int | None = None) -> dict:
        return {b.name: b for b in self.bufs(self.count if count is None else count, self.fmts[0] if fmt is None else fmt, **self.dims)}

    def device_bytes(self, fmt: str | None = None) -> int:
        return sum(b.alloc_bytes for b in self.buffers(fmt).values())

    def check_rows(self, fmt: str | None = None, rows: int | None = None) -> list:
        """Rows of the fp64 check: the first and last two, both sides of every boundary any row-indexed buffer crosses, every 4097th."""
        bufs = self.buffers(fmt)
        n = rows if rows is not None else max(b.rows for b in bufs.values() if b.role != "work")
        out = {0, 1, n - 2, n - 1} | set(range(0, n, EVERY))
        for b in bufs.values():
            if b.rows == n:
                out |= set(b.boundary_rows())
        return sorted(r for r in out if 0 <= r < n)


def planes_of(fmt: str) -> int:
    """Planes of an activation tensor in operand format `fmt` (tests/gpu_util.py planes_of, role "a")."""
    return 1 if fmt in ("bf16", "fp16") else 2


def first_crossing(pitch: int, boundary_elem: int, gran: int) -> int:
    """The smallest multiple of `gran` rows of `pitch` elements with an element AT index boundary_elem."""
    rows = boundary_elem // pitch + 1
    return (rows + gran - 1) // gran * gran


# ---- ragged lengths: 1861 (or more) sequences around 501 rows whose sum crosses with the LAST sequence -------------------------------------------
def seeded_lengths(nseq: int, lo: int, hi: int, need_rows: int) -> tuple:
    """(seed, lengths): nseq lengths drawn from lo .. hi with random.Random(seed), the first seed >= 0 whose lengths sum to at least need_rows
    while the first nseq - 1 of them do not -- the smallest batch of that draw that crosses."""
    for seed in range(10000):
        r = random.Random(seed)
        ln = [r.randint(lo, hi) for _ in range(nseq)]
        s = sum(ln)
        if s >= need_rows > s - ln[-1]:
            return seed, ln
    raise AssertionError("no seed below 10000 gives such lengths")


# ---- buffers per case ------------------------------------------------------------------------------------------------------------
def _split(numel, fmt, **_):
    npl = planes_of(fmt)
    return (Buf("src", numel // 1024, 1024, 4, role="in", fp32=True),
            Buf("dst", numel // 1024, 1024, 2, npl, "out", gap=GAP))


def _layernorm(rows, fmt, H, **_):
    return (Buf("x", rows, H, 4, role="in", fp32=True),
            Buf("out", rows, H, 2, planes_of(fmt), "out", gap=GAP))


def _gemm_out16(M, fmt, N, K, **_):
    npl = planes_of(fmt)
    return (Buf("A", M, K, 2, npl), Buf("out16", M, N, 2, npl, "out", gap=GAP), Buf("ref16", M, N, 2, npl, "ref", gap=GAP))


def _gemm_resid(M, fmt, N, K, **_):
    K = K[fmt] if isinstance(K, dict) else K
    return (Buf("A", M, K, 2, planes_of(fmt)), Buf("x0", M, N, 4, role="in", fp32=True),
            Buf("x_f32", M, N, 4, role="io", fp32=True, slack_rows=256), Buf("ref_f32", M, N, 4, role="ref", fp32=True))


def _rowln(M, fmt, K, **_):
    return (Buf("A", M, K, 2, 2), Buf("x0", M, 768, 4, role="in", fp32=True), Buf("x_f32", M, 768, 4, role="io", fp32=True, slack_rows=128),
            Buf("ref_f32", M, 768, 4, role="ref", fp32=True), Buf("out16", M, 768, 2, 2, "out", gap=GAP), Buf("ref16", M, 768, 2, 2, "ref"))


def _attention(nseq, fmt, H, S, lengths=None, **_):
    rows = nseq * S if lengths is None else sum(lengths[:nseq])
    npl = planes_of(fmt)
    return (Buf("qkv", rows, 3 * H, 2, npl, slack_rows=128),
            Buf("out", rows, H, 2, npl, "out", slack_rows=128), Buf("ref", rows, H, 2, npl, "ref", slack_rows=128))


def _rollout(nseq, fmt, H, S, lengths=None, **_):
    rows = nseq * S if lengths is None else sum(lengths[:nseq])
    smax = S if lengths is None else max(lengths)
    return (Buf("qkv", rows, 3 * H, 2, planes_of(fmt), slack_rows=128), Buf("r_in", rows, 1, 4, fp32=True),
            Buf("r_out", rows, 1, 4, role="out", fp32=True, gap=GAP), Buf("ref", rows, 1, 4, role="ref", fp32=True),
            Buf("part", rows, (H // 64) * ((smax + 127) // 128), 4, role="work", fp32=True))


def _probs(nseq, fmt, H, S, **_):
    nh = H // 64
    return (Buf("qkv", nseq * S, 3 * H, 2, planes_of(fmt)),
            Buf("probs", nseq * nh * S, S, 4, role="out", fp32=True, gap=GAP), Buf("ref", SLICE_SEQS * nh * S, S, 4, role="ref", fp32=True))


def _cls_fold(nseq, fmt, H, S, chunk_rows, lengths=None, **_):
    rows = nseq * S if lengths is None else sum(lengths[:nseq])
    smax = S if lengths is None else max(lengths)
    nh, r64 = H // 64, (nseq + 63) // 64 * 64
    return (Buf("x", rows, H, 4, fp32=True), Buf("q", nseq, H, 4, fp32=True), Buf("u", nseq * nh, H, 4, role="work", fp32=True),
            Buf("part", nseq * ((smax + chunk_rows - 1) // chunk_rows) * nh, H + 2, 4, role="work", fp32=True),
            Buf("z", r64, nh * H, 2, planes_of(fmt), "work"), Buf("ctx", nseq, H, 4, role="out", fp32=True, gap=GAP),
            Buf("ref", nseq, H, 4, role="ref", fp32=True))


def _images_uniform(NI, fmt, side, N, P, **_):
    return (Buf("images", NI * side, side * 3, 1), Buf("level0", NI * 3 * side, side, 4, role="out", fp32=True, gap=GAP),
            Buf("level1", NI * 3 * (side // 2), side // 2, 4, role="out", fp32=True, gap=GAP),
            Buf("ref0", 3 * side, side, 4, role="ref", fp32=True), Buf("ref1", 3 * (side // 2), side // 2, 4, role="ref", fp32=True),
            Buf("patches", NI * N, 3 * P * P, 4, role="out", fp32=True, gap=GAP))


# The ragged image gathers: three images in one byte buffer -- one at byte 0, one that straddles byte 2^32, one wholly behind it -- and
# nothing between them but the unfilled bytes of the buffer.  Sizes with odd sides, so that the second and third image start at odd bytes.
RAGGED_SIZES = ((331, 517), (419, 333), (263, 401))


def ragged_layout(esize: int) -> tuple:
    """(img_off [3], image_bytes) in bytes for pixel elements of `esize` bytes: image 1 starts so that byte 2^32 falls in its middle, image 2
    directly behind it; the buffer ends with image 2."""
    nb = [3 * h * w * esize for h, w in RAGGED_SIZES]
    off1 = ((1 << 32) - nb[1] // 2) // esize * esize
    if esize == 1:
        off1 |= 1                                 # an odd byte: the u8 gather takes any alignment
    off2 = off1 + nb[1]
    return (0, off1, off2), off2 + nb[2]


def _ragged(NI, fmt, N, P, **_):
    esize = {"u8": 1, "fp32": 4, "fp16": 2}[fmt]
    off, total = ragged_layout(esize)
    if NI < 3:                                    # one image fewer: the buffer ends with image NI - 1
        total = off[NI - 1] + 3 * RAGGED_SIZES[NI - 1][0] * RAGGED_SIZES[NI - 1][1] * esize
    return (Buf("images", total // esize, 1, esize, fp32=esize == 4), Buf("patches", NI * N, 3 * P * P, 4, role="out", fp32=True, gap=GAP),
            Buf("ref", NI * N, 3 * P * P, 4, role="ref", fp32=True))


def _engine(B, fmt, H, N, mlp, **_):
    rows = 2 * B * (N + 1)
    alloc = (rows + 255) // 256 * 256 + 128                  # engine.hip geometry_seq: M_pad + the attention slack
    npl = planes_of(fmt)
    return (Buf("patches", 2 * B * N, 768, 4, fp32=True), Buf("x", rows, H, 4, role="work", fp32=True, slack_rows=alloc - rows),
            Buf("lnbuf", rows, H, 2, npl, "work", slack_rows=alloc - rows), Buf("big", rows, mlp, 2, npl, "work", slack_rows=alloc - rows))


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
P16 = 1 << 31                                    # 16-bit buffers: 2^31 elements = 2^32 bytes, 2^30 elements = 2^31 bytes
ATT_ROWS = first_crossing(2304, P16, 1)           # rows of a [*, 3 * 768] plane that reach element 2^31: 932 068
VL_SEED, VL_LENGTHS = seeded_lengths(1861, 437, 565, ATT_ROWS)
FOLD_SEED, FOLD_LENGTHS = seeded_lengths(5582, 437, 565, first_crossing(768, P16, 1))
CHUNK_ROWS = 64                                  # vtq_k_cls_fold_chunk_rows(); the GPU test asserts it


def _cases():
    both = ("fp16x3", "bf16")
    c16 = (E31, B31, B32)                        # what a 16-bit plane behind 2^31 elements crosses
    return [
        Case("split", ("vtq_k_split",), both, (1 << 31) + (1 << 20), 1 << 20, "2^20 elements (the test's chunk)", ("src", E31),
             {"src": (E30, E31, B31, B32), "dst": c16}, _split, {}),
        Case("layernorm_768", ("vtq_k_layernorm",), ("fp16x3",), first_crossing(768, P16, 4), 4, "4 rows (one workgroup)", ("x", E31),
             {"x": (E30, E31, B31, B32), "out": c16}, _layernorm, dict(H=768)),
        Case("layernorm_1024", ("vtq_k_layernorm",), ("bf16",), first_crossing(1024, P16, 4), 4, "4 rows (one workgroup)", ("x", E31),
             {"x": (E30, E31, B31, B32), "out": c16}, _layernorm, dict(H=1024)),
        Case("gemm_fc1", ("vtq_k_gemm",), both, first_crossing(3072, P16, 256), 256, "one 256-row tile", ("out16", E31),
             {"out16": c16, "ref16": c16}, _gemm_out16, dict(N=3072, K=768, epilogues=(0, 1), tiles=(-1, 0, 1, 2, 3))),
        Case("gemm_fc2", ("vtq_k_gemm",), both, first_crossing(3072, P16, 256), 256, "one 256-row tile", ("A", E31),
             {"A": c16, "x0": (B31,), "x_f32": (B31,), "ref_f32": (B31,)}, _gemm_resid, dict(N=768, K=3072, tiles=(-1, 0, 1, 2, 3))),
        Case("gemm_tall_x", ("vtq_k_gemm",), both, first_crossing(768, 1 << 30, 256), 256, "one 256-row tile", ("x_f32", B32),
             {n: (E30, B31, B32) for n in ("x0", "x_f32", "ref_f32")}, _gemm_resid,
             dict(N=768, K={"fp16x3": 64, "bf16": 128}, tiles=(-1, 0, 1, 2, 3))),
        Case("rowln", ("vtq_k_gemm_rowln",), ("fp16x3", "bf16x3"), first_crossing(3072, P16, 128), 128, "one 128-row panel", ("A", E31),
             {"A": c16, "x0": (B31,), "x_f32": (B31,), "ref_f32": (B31,)}, _rowln, dict(K=3072)),
        Case("attention", ("vtq_k_attention",), both, 1861, 1, "one sequence", ("qkv", E31), {"qkv": c16}, _attention,
             dict(H=768, S=501, variants=(0, 1, 2))),
        Case("attention_varlen", ("vtq_vl_attention",), both, 1861, 1, "one sequence", ("qkv", E31), {"qkv": c16}, _attention,
             dict(H=768, S=501, lengths=VL_LENGTHS)),
        Case("rollout_step", ("vtq_k_rollout_step",), both, 1861, 1, "one sequence", ("qkv", E31), {"qkv": c16}, _rollout, dict(H=768, S=501)),
        Case("rollout_step_varlen", ("vtq_vl_rollout_step",), both, 1861, 1, "one sequence", ("qkv", E31), {"qkv": c16}, _rollout,
             dict(H=768, S=501, lengths=VL_LENGTHS)),
        Case("probs", ("vtq_k_attention_probs",), both, 713, 1, "one sequence", ("probs", E31), {"probs": (E30, E31, B31, B32)}, _probs,
             dict(H=768, S=501)),
        Case("cls_fold", ("vtq_k_cls_fold",), both, 5582, 1, "one sequence", ("x", E31), {"x": (E30, E31, B31, B32)}, _cls_fold,
             dict(H=768, S=501, chunk_rows=CHUNK_ROWS)),
        Case("cls_fold_varlen", ("vtq_vl_cls_fold",), both, 5582, 1, "one sequence", ("x", E31), {"x": (E30, E31, B31, B32)}, _cls_fold,
             dict(H=768, S=501, chunk_rows=CHUNK_ROWS, lengths=FOLD_LENGTHS)),
        Case("images_uniform", ("vtq_k_image_normalize", "vtq_k_avgpool2", "vtq_k_gather_patches"), ("",), 11, 1, "one image", ("level0", E31),
             {"images": (E31, B31), "level0": (E30, E31, B31, B32), "level1": (B31,)}, _images_uniform, dict(side=8192, N=8, P=16)),
        Case("images_ragged_u8", ("vtq_k_gather_patches_u8",), ("u8",), 3, 0, "one image", ("images", B32),
             {"images": (E31, B31, B32)}, _ragged, dict(N=12, P=16)),
        Case("images_planar_fp32", ("vtq_k_gather_patches_planar",), ("fp32",), 3, 0, "one image", ("images", B32),
             {"images": (E30, B31, B32)}, _ragged, dict(N=12, P=16)),
        Case("images_planar_fp16", ("vtq_k_gather_patches_planar",), ("fp16",), 3, 0, "one image", ("images", B32),
             {"images": (E31, B31, B32)}, _ragged, dict(N=12, P=16)),
        Case("engine", ("VTAMIQ.forward",), both, 698, 1, "one pair", ("big", E31), {"big": c16, "x": (B31,)}, _engine,
             dict(H=768, N=500, mlp=3072, slice_pairs=64)),
    ]


CASES = {c.name: c for c in _cases()}

# Entries of include/*.h that take a row, sequence, element or image count and have NO case, each with its reason.  An entry that is in
# neither table fails tests/test_large_offsets_plan.py.
EXCLUDED = {
    "vtq_k_skinny_linear": "one row per sequence (R <= the call's sequence count): a plane of R x 3072 crosses at about 7e5 sequences per call",
    "vtq_k_diffnet_head": "one row per scored image, on vtq_k_skinny_linear's stages: the same 7e5 images per call",
    "vtq_k_repeat_mean": "validation reduction over N <= 1e5 scores by design",
    "vtq_k_rank_metrics": "validation reduction over N <= 1e5 scores by design (its pair kernel is O(N^2))",
    "vtq_k_sample_grid": "refuses totals above 2^31 - 1 samples; tests/test_gpu_sampler.py covers the refusal",
    "vtq_k_diff_cells": "refuses tables above 2^31 - 1 words; tests/test_gpu_weighted_sampler.py covers the refusal",
    "vtq_k_sample_weighted": "refuses totals above 2^31 - 1 samples; tests/test_gpu_weighted_sampler.py covers the refusal",
    "vtq_k_quant_rows_fp8": "the fp8 experiment only (include/vtamiq_hip_fp8.h), not the product library",
    "vtq_k_quant_fp8": "the fp8 experiment only",
    "vtq_k_gemm_fp8": "the fp8 experiment only",
}
# host-only entries: no device buffer at all
HOST_ONLY = {"vtq_k_gemm_tile_rule", "vtq_k_attention_rule", "vtq_k_gemm_schedule", "vtq_k_cls_fold_chunk_rows", "vtq_vl_attention_blocks"}
