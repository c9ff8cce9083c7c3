"""Patch coordinates sampled on the GPU (include/vtamiq_hip_sampler.h, csrc/patch_sampler.hip): the reference's default sampler,
PatchSampler(grid_type=GRID_TYPE_PERTURBED_SIMPLE) (data/patch_sampling.py:308-395), with the per-image level and count arithmetic of
get_iqa_patches (data/patch_sampling.py:398-447, 511-512, 554-555) on the host and everything random on the device.

    samples, scale_ids, lengths = sample_patches(sizes, 500, keys, seed=0, device="cuda")
    patches, pos, scales = extract_patches_varlen(flat_u8, samples, lengths, scale_ids, sizes=sizes, validate=False)

The samples are a pure function of (seed, key, image size, patch count): one key for two images of one size is aligned sampling.  They are
in range by construction, so the gather needs no host check; the header states the definition and the two differences from the reference.
pipeline.ImagePairVarlenPipeline.submit_images / submit_group_images run this inside the pipeline's slots."""
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
