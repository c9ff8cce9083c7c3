"""Patch coordinates sampled on the GPU (include/vtamiq_hip_sampler.h, csrc/patch_sampler.hip): the reference's default sampler,
PatchSampler(grid_type=GRID_TYPE_PERTURBED_SIMPLE) (data/patch_sampling.py:308-395), with the per-image level and count arithmetic of
get_iqa_patches (data/patch_sampling.py:398-447, 511-512, 554-555) on the host and everything random on the device.

    samples, scale_ids, lengths = sample_patches(sizes, 500, keys, seed=0, device="cuda")
    patches, pos, scales = extract_patches_varlen(flat_u8, samples, lengths, scale_ids, sizes=sizes, validate=False)

The samples are a pure function of (seed, key, image size, patch count): one key for two images of one size is aligned sampling.  They are
in range by construction, so the gather needs no host check; the header states the definition and the two differences from the reference.
pipeline.ImagePairVarlenPipeline.submit_images / submit_group_images run this inside the pipeline's slots.

WeightedPatchSampler / sample_patches_weighted (include/vtamiq_hip_weighted_sampler.h, csrc/patch_sampler_weighted.hip) are the reference's
PatchSampler(diff_weight > 0, grid_type=GRID_TYPE_PERTURBED): a difference pass over the resident bytes of a pair, then a sampler that
places the patches where the pair differs; submit_images(..., sampler=WeightedPatchSampler(...)) runs both in the slots."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

# the reference's constants (data/patch_sampling.py:17-25)
GRID_TYPE_HALTON = 0
GRID_TYPE_PERTURBED = 1
GRID_TYPE_PERTURBED_SIMPLE = 2
DIFF_TYPE_MAGNITUDE = 0
DIFF_TYPE_DARK = 1
DEFAULT_NUM_SAMPLES_RATIO = 1.7
GRID_TYPE_PERTURBED_AMOUNT = 0.2

MAX_CELLS = 8192            # VTQ_SAMPLER_MAX_CELLS: grid cells of one (image, level)
MAX_EXTENT = 1 << 26        # VTQ_SAMPLER_MAX_EXTENT
MAX_LEVELS = 4
_M64 = (1 << 64) - 1


def quantise_amount(perturbed_amount: float) -> int:
    """perturbed_amount -> the 16-bit fixed-point factor the kernel multiplies by (0.2 -> 13107)."""
    q = int(round(float(perturbed_amount) * 65536.0))
    if not 0 <= q <= 65535:
        raise ValueError(f"perturbed_amount={perturbed_amount}: 0 <= amount < 1 (16-bit fixed point)")
    return q


class PatchSampler:
    """The reference's constructor keywords.  Built: the uniform GRID_TYPE_PERTURBED_SIMPLE grid; the rest is refused by name."""

    def __init__(self, centerbias_weight=0.0, diff_weight=0.0, uniform_weight=1.0, grid_type=GRID_TYPE_PERTURBED_SIMPLE,
                 diff_type=DIFF_TYPE_MAGNITUDE, perturbed_amount=GRID_TYPE_PERTURBED_AMOUNT):
        if grid_type == GRID_TYPE_PERTURBED:
            raise NotImplementedError("GRID_TYPE_PERTURBED is not built: only GRID_TYPE_PERTURBED_SIMPLE is sampled on the device")
        if grid_type == GRID_TYPE_HALTON:
            raise NotImplementedError("GRID_TYPE_HALTON is not built: only GRID_TYPE_PERTURBED_SIMPLE is sampled on the device")
        if grid_type != GRID_TYPE_PERTURBED_SIMPLE:
            raise ValueError("Unsupported grid function type.")
        if diff_weight > 0:
            raise NotImplementedError("diff_weight > 0 is not built (the reference's SIMPLE grid ignores it too, with a warning): pass 0")
        if centerbias_weight > 0:
            raise NotImplementedError("centerbias_weight > 0 is not built (the reference's SIMPLE grid ignores it too, with a warning): pass 0")
        if max(0.0, uniform_weight) < 1e-6:
            raise ValueError("Total weight must be non-zero.")
        self.centerbias_weight, self.diff_weight, self.uniform_weight = 0.0, 0.0, max(0.0, uniform_weight)
        self.grid_type, self.diff_type, self.perturbed_amount = grid_type, diff_type, perturbed_amount
        self.amount_q = quantise_amount(perturbed_amount)


def compute_patch_num_scales(patch_num_scales: int, h: int, w: int, ho: int, wo: int) -> int:
    """How many levels an h x w image gets when patch_num_scales are asked for (data/patch_sampling.py:398-411, restated)."""
    if patch_num_scales <= 1:
        return 1
    dim, possible = min(h, w), 0
    while 1 < dim:
        possible += 1
        dim = (dim - max(ho, wo)) / 2
    return max(1, min(possible - 1, patch_num_scales))


def compute_num_patches_per_scale(patch_count: int, patch_num_scales: int, scale_num_samples_ratio: float) -> np.ndarray:
    """Patch counts per level, COARSEST level first as in the reference (data/patch_sampling.py:427-447, restated): level s gets entry -1 - s."""
    num = 2 ** (scale_num_samples_ratio * np.arange(patch_num_scales))
    num = np.ceil(num * patch_count / np.sum(num)).astype(int)
    cum = np.cumsum(num)
    for i in range(patch_num_scales):
        if patch_count <= cum[i]:
            num[i] -= cum[i] - patch_count
            num[i + 1:] = 0
            break
    return num


def grid_dims(n: int, h: int, w: int):
    """(Hg, Wg) of n samples on an h x w level, in fp64 exactly as numpy computes them in the reference (data/patch_sampling.py:308, 322-324)."""
    aspect = h / w
    wg = np.maximum(np.ceil(np.sqrt(np.array([n]) / aspect)), 1.)
    hg = np.ceil(wg * aspect)
    return int(hg[0]), int(wg[0])


class SamplePlan(NamedTuple):
    """What the host knows about a batch's samples without drawing any (plan_samples)."""
    lengths: np.ndarray       # int64 [NI] patches per image
    seg: np.ndarray           # int32 [NS, 8] = (first row, n, Hg, Wg, h - P, w - P, level, 0): the kernel's segment table
    seg_image: np.ndarray     # int32 [NS] the image of every segment
    levels: list              # NI level counts (the reference's rule)
    total: int


def patch_counts(patch_count, n: int) -> list:
    """patch_count as n ints: one int for all n images (or pairs), or n of them."""
    counts = [int(patch_count)] * n if np.ndim(patch_count) == 0 else [int(c) for c in patch_count]
    if len(counts) != n:
        raise ValueError(f"patch_count: one int, or one per pair / image ({n})")
    return counts


def plan_samples(sizes, patch_count, num_scales: int = 1, scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO,
                 patch_size: int = 16) -> SamplePlan:
    """Host side of the sampler, numpy only.  sizes: NI (H, W); patch_count: one int for all images or NI ints.  Image i gets the
    reference's level count for its size, its patch_count split over those levels by the reference's rule, and one segment per level that
    has patches, level 0 first: rows [first, first + n) of the batch's sample list.  ValueError for an image smaller than a patch, a patch
    count below num_scales (get_iqa_patches refuses that) and a level whose grid exceeds MAX_CELLS = 8192 cells."""
    P = int(patch_size)
    if not 1 <= num_scales <= MAX_LEVELS:
        raise ValueError("1 <= num_scales <= 4")
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not sizes:
        raise ValueError("sizes: at least one (H, W)")
    counts = patch_counts(patch_count, len(sizes))
    rows, seg_image, levels, first = [], [], [], 0
    for i, ((h, w), count) in enumerate(zip(sizes, counts)):
        if h < P or w < P:
            raise ValueError(f"image {i} ({h}x{w}) is smaller than one {P}x{P} patch")
        if count < max(1, num_scales):
            raise ValueError(f"image {i}: patch_count={count} is below num_scales={num_scales} (at least one patch per scale asked for)")
        L = compute_patch_num_scales(num_scales, h, w, P, P)
        per_level = compute_num_patches_per_scale(count, L, scale_num_samples_ratio)
        levels.append(L)
        for s in range(L):
            n = int(per_level[-1 - s])
            if n < 1:
                continue
            hs, ws = h >> s, w >> s
            hg, wg = grid_dims(n, hs, ws)
            if hg * wg > MAX_CELLS:
                raise ValueError(f"image {i}, level {s}: {n} samples need a grid of {hg} x {wg} cells, the sampler takes {MAX_CELLS} per level")
            if hs - P >= MAX_EXTENT or ws - P >= MAX_EXTENT:
                raise ValueError(f"image {i}: a level of {hs} x {ws} pixels is beyond the sampler's {MAX_EXTENT}")
            rows.append((first, n, hg, wg, hs - P, ws - P, s, 0))
            seg_image.append(i)
            first += n
    if first > 0x7fffffff:
        raise ValueError("more than 2^31 - 1 samples")
    return SamplePlan(np.asarray(counts, np.int64), np.asarray(rows, np.int32).reshape(-1, 8), np.asarray(seg_image, np.int32), levels, first)


def as_keys(keys, n: int) -> np.ndarray:
    """n 64-bit keys as uint64 (Python ints of any sign are taken mod 2^64)."""
    k = np.asarray([int(x) & _M64 for x in np.asarray(keys, dtype=object).reshape(-1)], dtype=np.uint64)
    if k.shape != (n,):
        raise ValueError(f"keys: {n} expected, {k.shape[0]} given")
    return k


def repeat_key(key: int, r: int) -> int:
    """The key of validation repeat r of the pair / image with `key`: the key itself for r = 0, else the splitmix64 finaliser (Steele,
    Lea, Flood 2014; Vigna) of key + r * 0x9e3779b97f4a7c15, mod 2^64."""
    key = int(key) & _M64
    if r == 0:
        return key
    z = (key + r * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def launch_sample_grid(dev_seg: torch.Tensor, dev_keys: torch.Tensor, seg: np.ndarray, seg_keys: np.ndarray, seed: int, amount_q: int,
                       samples: torch.Tensor, scale_ids: Optional[torch.Tensor]) -> None:
    """The launch itself (vtq_k_sample_grid) on the current stream: dev_seg / dev_keys are the device copies of the host arrays seg
    (int32 [NS, 8]) / seg_keys (uint64 [NS]), samples / scale_ids the device outputs.  Nothing here copies or synchronises."""
    lib = _lib.load()
    dev = samples.device
    with torch.cuda.device(dev):
        _lib.check(lib.vtq_k_sample_grid(dev_seg.data_ptr(), dev_keys.data_ptr(), seg.ctypes.data_as(C.POINTER(C.c_int32)),
                                         seg_keys.ctypes.data_as(C.POINTER(C.c_uint64)), seg.shape[0], int(seed) & _M64, int(amount_q),
                                         samples.data_ptr(), scale_ids.data_ptr() if scale_ids is not None else None,
                                         torch.cuda.current_stream(dev).cuda_stream))


def sample_patches(sizes, patch_count, keys, seed: int = 0, num_scales: int = 1,
                   scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO, patch_size: int = 16,
                   sampler: Optional[PatchSampler] = None, device=None, randomize_patch_scale_order: bool = False):
    """Sample patch_count patches on each of the NI images of `sizes` with one 64-bit key per image.  Returns (samples int32 (total, 2),
    scale_ids int32 (total,) or None when num_scales == 1, lengths: list of NI ints), the tensors on `device`, concatenated per image with
    level 0 first: what extract_patches_varlen(..., validate=False) takes.  Equal (key, size, count) give equal rows."""
    if randomize_patch_scale_order:
        raise NotImplementedError("randomize_patch_scale_order=True is not built: patches are ordered by scale, level 0 first")
    sampler = sampler if sampler is not None else PatchSampler()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("sample_patches runs on the GPU only (no CPU fallback on the product path)")
    plan = plan_samples(sizes, patch_count, num_scales, scale_num_samples_ratio, patch_size)
    seg = np.ascontiguousarray(plan.seg)
    seg_keys = np.ascontiguousarray(as_keys(keys, len(plan.lengths))[plan.seg_image])
    dev_seg = torch.from_numpy(seg).to(dev)
    dev_keys = torch.from_numpy(seg_keys.view(np.int64)).to(dev)
    samples = torch.empty(plan.total, 2, dtype=torch.int32, device=dev)
    scale_ids = torch.empty(plan.total, dtype=torch.int32, device=dev) if num_scales > 1 else None
    launch_sample_grid(dev_seg, dev_keys, seg, seg_keys, seed, sampler.amount_q, samples, scale_ids)
    return samples, scale_ids, plan.lengths.tolist()


# ---- patches placed where a pair differs (include/vtamiq_hip_weighted_sampler.h, csrc/patch_sampler_weighted.hip) ---------------------------
MAX_SAMPLES_WEIGHTED = 8100     # VTQ_WSAMPLER_MAX_SAMPLES: samples of one (image, level)
MAX_PIXELS_WEIGHTED = 1 << 22   # VTQ_WSAMPLER_MAX_PIXELS: H * W of one image


class WeightedPatchSampler:
    """The reference's PatchSampler(grid_type=GRID_TYPE_PERTURBED, diff_weight, uniform_weight): stratified cells that get samples in
    proportion to diff_weight * (the pair's difference over the cell's window, in units of its standard deviation) + uniform_weight * (the
    window's area), a perturbed sub-grid inside every cell.  diff_weight = 0 is the uniform GRID_TYPE_PERTURBED grid.  Built:
    DIFF_TYPE_MAGNITUDE with diff_pow = 1; the rest is refused by name.  sampling.PatchSampler keeps the SIMPLE grid and its refusals."""
    grid_type = GRID_TYPE_PERTURBED

    def __init__(self, diff_weight=0.0, uniform_weight=1.0, perturbed_amount=GRID_TYPE_PERTURBED_AMOUNT, diff_type=DIFF_TYPE_MAGNITUDE,
                 centerbias_weight=0.0):
        if centerbias_weight > 0:
            raise NotImplementedError("centerbias_weight > 0 is not built (the reference's template file is not part of its tree): pass 0")
        if diff_type == DIFF_TYPE_DARK and diff_weight > 0:
            raise NotImplementedError("DIFF_TYPE_DARK is not built: only DIFF_TYPE_MAGNITUDE weights the samples")
        if diff_type not in (DIFF_TYPE_MAGNITUDE, DIFF_TYPE_DARK):
            raise ValueError("Unsupported diff type.")
        self.diff_weight, self.uniform_weight = max(0.0, float(diff_weight)), max(0.0, float(uniform_weight))
        if not np.isfinite(self.diff_weight + self.uniform_weight) or self.diff_weight + self.uniform_weight < 1e-6:
            raise ValueError("Total weight must be non-zero.")
        self.centerbias_weight, self.diff_type, self.perturbed_amount = 0.0, diff_type, perturbed_amount
        self.amount_q = quantise_amount(perturbed_amount)


def cell_geometry(n: int, h: int, w: int, P: int):
    """(cs, sh, sw): cell size and cell counts of n samples on an h x w level, in fp64 exactly as numpy computes them in the reference
    (data/patch_sampling.py:240-253); a level exactly P high or wide keeps one row or column of cells of extent 0."""
    cs = int(max(0.75 * P, min(max(h, w) / P * 3., np.sqrt(h * w / n * 4.))))
    return cs, max(1, int(np.ceil((h - P) / cs))), max(1, int(np.ceil((w - P) / cs)))


class WeightedPlan(NamedTuple):
    """What the host knows about a batch's weighted samples without reading a pixel (plan_samples_weighted)."""
    lengths: np.ndarray       # int64 [NI] patches per image
    seg: np.ndarray           # int32 [NS, 12] = (first row, n, cs, sh, sw, h - P, w - P, level, head, tab_off, 0, 0): the sampler's table
    seg_image: np.ndarray     # int32 [NS] the image of every segment
    pairs: np.ndarray         # int64 [NP, 8] = (a_off, b_off, H, W, head, first lev row, lev rows, 0); the caller fills the two offsets
    lev: np.ndarray           # int32 [NL, 8] = (pair, level, cs, sh, sw, head, tab_off, 0): the difference pass's table
    tab_words: int            # uint64 words of the weight table
    total: int


def plan_samples_weighted(sizes, patch_count, num_scales: int = 1, scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO,
                          patch_size: int = 16, pair_of=None) -> WeightedPlan:
    """Host side of the weighted sampler, numpy only: geometry and tables.  sizes: NI (H, W); patch_count: one int or NI; pair_of: the
    pair whose weight table image i is sampled from (default: image i has table i), pairs numbered 0 .. NP - 1 -- every image of a pair
    needs the pair's size and patch count, since the cells depend on both.  Levels, counts per level and segment order are those of
    plan_samples.  ValueError for what plan_samples refuses, for a level with more than 8192 cells or 8100 samples and for an image
    above 2^22 pixels."""
    P = int(patch_size)
    if not 8 <= P <= 64:
        raise ValueError("8 <= patch_size <= 64")
    if not 1 <= num_scales <= MAX_LEVELS:
        raise ValueError("1 <= num_scales <= 4")
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not sizes:
        raise ValueError("sizes: at least one (H, W)")
    counts = patch_counts(patch_count, len(sizes))
    pair_of = list(range(len(sizes))) if pair_of is None else [int(p) for p in pair_of]
    NP = max(pair_of) + 1
    if len(pair_of) != len(sizes) or sorted(set(pair_of)) != list(range(NP)):
        raise ValueError("pair_of: one pair per image, pairs numbered 0 .. NP - 1 without gaps")
    per_image, pair_rows = [], {}
    for i, ((h, w), count) in enumerate(zip(sizes, counts)):
        if h < P or w < P:
            raise ValueError(f"image {i} ({h}x{w}) is smaller than one {P}x{P} patch")
        if h * w > MAX_PIXELS_WEIGHTED:
            raise ValueError(f"image {i} ({h}x{w}) has more than 2^22 pixels, the difference pass's limit")
        if count < max(1, num_scales):
            raise ValueError(f"image {i}: patch_count={count} is below num_scales={num_scales} (at least one patch per scale asked for)")
        L = compute_patch_num_scales(num_scales, h, w, P, P)
        per_level = compute_num_patches_per_scale(count, L, scale_num_samples_ratio)
        rows = []
        for s in range(L):
            n = int(per_level[-1 - s])
            if n < 1:
                continue
            if n > MAX_SAMPLES_WEIGHTED:
                raise ValueError(f"image {i}, level {s}: {n} samples, the weighted sampler takes {MAX_SAMPLES_WEIGHTED} per level")
            hs, ws = h >> s, w >> s
            cs, sh, sw = cell_geometry(n, hs, ws, P)
            if sh * sw > MAX_CELLS:
                raise ValueError(f"image {i}, level {s}: {sh} x {sw} cells, the sampler takes {MAX_CELLS} per level")
            rows.append((n, cs, sh, sw, hs - P, ws - P, s))
        per_image.append(rows)
        if pair_rows.setdefault(pair_of[i], ((h, w), rows)) != ((h, w), rows):
            raise ValueError(f"image {i} differs from the other image of pair {pair_of[i]} in size or patch count: the pair has one table")
    pairs, lev, where, T = np.zeros((NP, 8), np.int64), [], {}, 0
    for p in range(NP):
        (h, w), rows = pair_rows[p]
        pairs[p, 2:7] = (h, w, T, len(lev), len(rows))
        head, T = T, T + 4
        for n, cs, sh, sw, hm, wm, s in rows:
            lev.append((p, s, cs, sh, sw, head, T, 0))
            where[(p, s)] = (head, T)
            T += 2 + sh * sw
    if T > 0x7fffffff:
        raise ValueError("a weight table above 2^31 - 1 words")
    seg, seg_image, first = [], [], 0
    for i, rows in enumerate(per_image):
        for n, cs, sh, sw, hm, wm, s in rows:
            seg.append((first, n, cs, sh, sw, hm, wm, s) + where[(pair_of[i], s)] + (0, 0))
            seg_image.append(i)
            first += n
    if first > 0x7fffffff:
        raise ValueError("more than 2^31 - 1 samples")
    return WeightedPlan(np.asarray(counts, np.int64), np.asarray(seg, np.int32).reshape(-1, 12), np.asarray(seg_image, np.int32), pairs,
                        np.asarray(lev, np.int32).reshape(-1, 8), T, first)


def segments_for(plan: WeightedPlan, sampler: WeightedPatchSampler) -> np.ndarray:
    """The plan's segment table as the sampler entry takes it for `sampler`: with diff_weight == 0 there is no weight table (no pixel is
    read, tab is NULL), so no segment may point into one -- head = tab_off = -1."""
    seg = np.ascontiguousarray(plan.seg).copy()
    if not sampler.diff_weight > 0:
        seg[:, 8:10] = -1
    return seg


def launch_diff_cells(flat: torch.Tensor, dev_pairs: torch.Tensor, dev_lev: torch.Tensor, pairs: np.ndarray, lev: np.ndarray,
                      patch_size: int, tab: torch.Tensor, tab_words: int) -> None:
    """The difference pass (vtq_k_diff_cells) on the current stream: flat the uint8 image buffer, dev_pairs / dev_lev the device copies of
    the host arrays pairs (int64 [NP, 8]) / lev (int32 [NL, 8]), tab the int64 device tensor whose first tab_words words are written.
    Nothing here copies or synchronises."""
    lib = _lib.load()
    dev = flat.device
    with torch.cuda.device(dev):
        _lib.check(lib.vtq_k_diff_cells(flat.data_ptr(), flat.numel(), dev_pairs.data_ptr(), dev_lev.data_ptr(),
                                        pairs.ctypes.data_as(C.POINTER(C.c_int64)), lev.ctypes.data_as(C.POINTER(C.c_int32)), pairs.shape[0],
                                        lev.shape[0], int(patch_size), tab.data_ptr(), int(tab_words), torch.cuda.current_stream(dev).cuda_stream))


def launch_sample_weighted(dev_seg: torch.Tensor, dev_keys: torch.Tensor, seg: np.ndarray, seg_keys: np.ndarray, patch_size: int,
                           tab: Optional[torch.Tensor], tab_words: int, sampler: WeightedPatchSampler, seed: int, samples: torch.Tensor,
                           scale_ids: Optional[torch.Tensor]) -> None:
    """The weighted sampler (vtq_k_sample_weighted) on the current stream; the arguments as launch_sample_grid's, seg int32 [NS, 12]."""
    lib = _lib.load()
    dev = samples.device
    with torch.cuda.device(dev):
        _lib.check(lib.vtq_k_sample_weighted(dev_seg.data_ptr(), dev_keys.data_ptr(), seg.ctypes.data_as(C.POINTER(C.c_int32)),
                                             seg_keys.ctypes.data_as(C.POINTER(C.c_uint64)), seg.shape[0], int(patch_size),
                                             tab.data_ptr() if tab is not None else None, int(tab_words), sampler.diff_weight,
                                             sampler.uniform_weight, int(seed) & _M64, sampler.amount_q, samples.data_ptr(),
                                             scale_ids.data_ptr() if scale_ids is not None else None,
                                             torch.cuda.current_stream(dev).cuda_stream))


def sample_patches_weighted(images: torch.Tensor, img_off, sizes, patch_count, keys, sampler: WeightedPatchSampler, seed: int = 0,
                            num_scales: int = 1, scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO, patch_size: int = 16,
                            aligned: bool = True):
    """Sample patch_count patches on both images of each of B pairs.  images: ONE flat uint8 cuda tensor; img_off: the 2B byte offsets of
    the images in it, the B references first; sizes: B (H, W), a pair's two images have one size; keys: B (aligned: both images of a pair
    get the same rows) or 2B, references first.  Returns (samples int32 (total, 2), scale_ids int32 (total,) or None when num_scales == 1,
    lengths: 2B ints), per image, references first: what extract_patches_varlen(..., validate=False) takes.  With diff_weight == 0 no
    pixel is read."""
    if not isinstance(sampler, WeightedPatchSampler):
        raise TypeError("sample_patches_weighted takes a WeightedPatchSampler")
    if not isinstance(images, torch.Tensor) or images.device.type != "cuda" or images.dtype != torch.uint8 or images.dim() != 1:
        raise RuntimeError("sample_patches_weighted takes one flat uint8 tensor on the GPU (no CPU fallback on the product path)")
    dev = images.device
    sizes = [(int(h), int(w)) for h, w in sizes]
    B = len(sizes)
    off = [int(o) for o in img_off]
    if len(off) != 2 * B:
        raise ValueError("img_off: 2B byte offsets, references first")
    counts = patch_counts(patch_count, B)
    plan = plan_samples_weighted(sizes * 2, counts * 2, num_scales, scale_num_samples_ratio, patch_size, pair_of=list(range(B)) * 2)
    k = as_keys(keys, B if aligned else 2 * B)
    k = np.concatenate([k, k]) if aligned else k
    pairs = plan.pairs.copy()
    pairs[:, 0], pairs[:, 1] = off[:B], off[B:]
    seg, lev = segments_for(plan, sampler), np.ascontiguousarray(plan.lev)
    seg_keys = np.ascontiguousarray(k[plan.seg_image])
    samples = torch.empty(plan.total, 2, dtype=torch.int32, device=dev)
    scale_ids = torch.empty(plan.total, dtype=torch.int32, device=dev) if num_scales > 1 else None
    tab = None
    if sampler.diff_weight > 0:
        tab = torch.empty(plan.tab_words, dtype=torch.int64, device=dev)
        launch_diff_cells(images, torch.from_numpy(pairs).to(dev), torch.from_numpy(lev).to(dev), pairs, lev, patch_size, tab, plan.tab_words)
    launch_sample_weighted(torch.from_numpy(seg).to(dev), torch.from_numpy(seg_keys.view(np.int64)).to(dev), seg, seg_keys, patch_size, tab,
                           plan.tab_words if tab is not None else 0, sampler, seed, samples, scale_ids)
    return samples, scale_ids, plan.lengths.tolist()
