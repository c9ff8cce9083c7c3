"""Scores for image tensors that are already on the GPU: the output of another model against its target, without leaving the device.

    metric = ImageMetric(model, patch_count=500)
    q = metric(ref, dist)                               # (B, 3, H, W) float tensors in [0, 1] on the device -> q (B,) on the device
    q = metric.group(refs, dists, ref_index)            # G references, M distorted images, image m against reference ref_index[m]

A float image is gathered as it is (patches.extract_patches_planar's kernel, include/vtamiq_hip_tensors.h): no quantisation to 8 bits --
which would discard exactly the sub-LSB differences an evaluation of codecs or restoration networks is about --, no permute to HWC and no
trip through the host.  Device-resident uint8 HWC images go through the u8 gather and get the bits ImagePairVarlenPipeline.submit_images
gives for the same images as host arrays.

One call is: sizes from the shapes, on the host -> sampling.plan_samples -> one small pinned upload per side (tables, segments, keys) ->
sampling.launch_sample_grid into a device sample buffer -> the gather, one launch per side -> forward_varlen, or forward_group(lengths=)
for group().  Everything is enqueued on the current stream; no device value is read back and nothing synchronises.  Each of those steps
is the pipeline's own function: this module composes them and states none of their checks again."""
from __future__ import annotations

import warnings
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from .patches import ImageTables, ResidentImages, _gather, image_tables, resident_images, table_rows
from .pipeline import (BlockLayout, _aligned_sizes, _ref_indices, _sides, block_layout, default_keys, mean_over_repeats, pair_keys,
                       repeat_keys)
from .sampling import (DEFAULT_NUM_SAMPLES_RATIO, PatchSampler, WeightedPatchSampler, as_keys, launch_sample_grid, patch_counts, plan_samples,
                       plan_samples_weighted, sample_patches_weighted)


class _Side(NamedTuple):
    """One side of a call (references or distorted images) as the host plans it: its images num_repeats times, repeat-major."""
    tables: ImageTables       # R * n table rows; the rows of repeat r > 0 point at the pixels of repeat 0
    seg: np.ndarray           # int32 [NS, 8]  sampling.plan_samples over those rows
    seg_keys: np.ndarray      # uint64 [NS]
    layout: BlockLayout       # the side's device block: tab | patch_img | seg | keys uploaded, samples | scale ids written by the sampler
    lengths: list             # R * n patch counts


class ImageMetric:
    """model: a VTAMIQ on the GPU, in eval mode.  patch_count: patches per image, one int or one per pair (group(): per reference);
    num_scales: pyramid levels asked for (an image uses those it can hold); num_repeats=R: every pair is scored R times with the keys
    sampling.repeat_key(key, r) and the R scores are averaged on the device (validate.average_over_repeats: fp64 then), as
    submit_images does; seed, sampler (sampling.PatchSampler, the reference's default grid) and scale_num_samples_ratio as in
    sampling.sample_patches; mean, std: the normalisation of the gather, (x - mean[c]) / std[c] for pixels in [0, 1] -- a uint8 byte
    is divided by 255 first.

    The samples are a pure function of (seed, key, image size, patch count); keys=None takes them from this metric's call counter, so
    every call samples new positions, and a caller who wants the same positions again passes its own keys."""

    def __init__(self, model, patch_count=500, num_scales: int = 1, num_repeats: int = 1, seed: int = 0,
                 mean: Sequence[float] = (0.5, 0.5, 0.5), std: Sequence[float] = (0.5, 0.5, 0.5), sampler: Optional[PatchSampler] = None,
                 scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO):
        if int(num_repeats) < 1:
            raise ValueError("num_repeats >= 1")
        if sampler is not None and not isinstance(sampler, (PatchSampler, WeightedPatchSampler)):
            raise TypeError("sampler: a sampling.PatchSampler (or None for the default)")
        self.model, self.patch_count = model, patch_count
        self.num_scales, self.num_repeats, self.seed = int(num_scales), int(num_repeats), int(seed)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("mean and std: three values each")
        self.sampler = sampler if sampler is not None else PatchSampler()
        self.ratio = scale_num_samples_ratio
        self.P = model.spec.patch_size
        self.count = 0                                       # calls enqueued; a refused call is not counted and enqueues nothing

    # ---- host side: nothing here touches the device ----------------------------------------------------------------------------------
    def _images(self, first, second, names):
        """Both sides inspected (patches.resident_images) and the refusals that concern the two together."""
        a, b = resident_images(first, None, names[0], u8=True), resident_images(second, None, names[1], u8=True)
        if a.dtype != b.dtype:
            raise TypeError(f"{names[0]} is {a.dtype} and {names[1]} is {b.dtype}: one dtype for both (convert one side; a silent conversion "
                            "here would score something else than what was passed)")
        if a.device != b.device:
            raise ValueError(f"{names[0]} and {names[1]} must live on one device")
        if isinstance(self.sampler, WeightedPatchSampler):
            if a.dtype != torch.uint8:
                raise NotImplementedError("WeightedPatchSampler with float images is not built: its integer pixel weight is defined on bytes "
                                          "(include/vtamiq_hip_weighted_sampler.h); use the default sampler")
            if names[0] == "refs":
                raise NotImplementedError("group() with WeightedPatchSampler is not built: a group has no pairs of one size to difference")
            if a.sizes != b.sizes:
                raise ValueError("WeightedPatchSampler: the two images of a pair must have one size (their difference is taken pixel by pixel)")
        if torch.is_grad_enabled() and any(t.requires_grad for t in a.parts + b.parts):
            warnings.warn("vtamiq_amd.ImageMetric returns scores without an autograd graph (inference engine): the images' requires_grad "
                          "has no effect")
        return a, b

    def _plan(self, res: ResidentImages, counts, keys) -> _Side:
        n, R = len(res.sizes), self.num_repeats
        rows = np.tile(np.arange(n), R)                      # the image of every table row
        lengths = np.asarray(counts, dtype=np.int64)[rows]
        plan = plan_samples([res.sizes[i] for i in rows], lengths.tolist(), self.num_scales, self.ratio, self.P)
        elem = torch.empty((), dtype=res.dtype).element_size()
        base = image_tables(res.sizes, counts, elem)
        if len(res.parts) == 1 and res.parts[0].numel() * elem != base.image_bytes:
            raise ValueError(f"the flat image tensor has {res.parts[0].numel() * elem} bytes, the sizes need {base.image_bytes}")
        tables = table_rows(base, rows, lengths)
        seg = np.ascontiguousarray(plan.seg)
        return _Side(tables, seg, np.ascontiguousarray(repeat_keys(keys, R)[plan.seg_image]),
                     block_layout(len(rows), tables.total, len(seg), self.num_scales > 1), lengths.tolist())

    # ---- device side: the current stream, no read-back ------------------------------------------------------------------------------
    def _sample(self, side: _Side, dev):
        """One pinned block up (tables, segments, keys), the sampler behind it: (tab, patch_img, samples, scale ids) on the device."""
        L = side.layout
        host = torch.empty(L.uploaded, dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[L.tab], h[L.patch_img], h[L.patch_img.stop:L.seg.start] = side.tables.tab.reshape(-1), side.tables.patch_img, 0
        h[L.seg], h[L.keys] = side.seg.reshape(-1), side.seg_keys.view(np.int32)
        block = torch.empty(L.words, dtype=torch.int32, device=dev)
        block[:L.uploaded].copy_(host, non_blocking=True)    # pinned: asynchronous; torch's host allocator keeps the block until the copy ran
        tab, pimg, seg, keys, smp, sid = L.split(block)
        launch_sample_grid(seg, keys, side.seg, side.seg_keys, self.seed, self.sampler.amount_q, smp, sid)
        return tab, pimg, smp, sid

    def _gather(self, res: ResidentImages, side: _Side, sampled):
        tab, pimg, smp, sid = sampled
        return _gather(res.flat(), side.tables, tab, pimg, smp, sid, None, self.num_scales, self.mean, self.std, self.P)

    def _patches(self, a, b, side_a: _Side, side_b: _Side, shared: bool):
        """(patches, pos, scales) of both sides, each a (first, second) pair.  shared: the two sides have the same sizes, counts and keys
        (aligned sampling), so their coordinates and tables are the same: sampled once, gathered twice."""
        with torch.cuda.device(a.device):
            sa = self._sample(side_a, a.device)
            sb = sa if shared else self._sample(side_b, a.device)
            oa, ob = self._gather(a, side_a, sa), self._gather(b, side_b, sb)
        self.count += 1
        return tuple((x, y) for x, y in zip(oa, ob))

    def _weighted(self, r: ResidentImages, d: ResidentImages, counts, kr, kd, aligned: bool) -> torch.Tensor:
        """__call__ with sampler=WeightedPatchSampler on uint8 images: the patches go where a pair's two images differ
        (sampling.sample_patches_weighted, no kernel of this module's own).  Its difference pass reads both images of a pair from ONE
        buffer, so the two sides are concatenated on the device (one copy of the images), and its tables are uploaded from pageable
        memory.  The num_repeats listings of a pair are pairs of their own to the sampler: R difference passes over the same pixels."""
        B, R = len(r.sizes), self.num_repeats
        rows = np.concatenate([np.tile(np.arange(B), R), np.tile(np.arange(B, 2 * B), R)])
        base = image_tables(r.sizes + d.sizes, counts + counts)
        tables = table_rows(base, rows, np.asarray(counts + counts, dtype=np.int64)[rows])
        keys = repeat_keys(kr, R) if aligned else np.concatenate([repeat_keys(kr, R), repeat_keys(kd, R)])
        args = (r.sizes * R, counts * R, keys.tolist(), self.sampler, self.seed, self.num_scales, self.ratio, self.P, aligned)
        plan_samples_weighted(args[0] * 2, args[1] * 2, self.num_scales, self.ratio, self.P, pair_of=list(range(B * R)) * 2)   # its refusals, first
        dev = r.device
        with torch.cuda.device(dev):
            flat = torch.cat([r.flat(), d.flat()])
            smp, sid, lengths = sample_patches_weighted(flat, tables.img_off, *args)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            out = _gather(flat, tables, up(tables.tab), up(tables.patch_img), smp, sid, None, self.num_scales, self.mean, self.std, self.P)
        self.count += 1
        first = lengths[:B * R]
        patches, pos, scales = _sides(out, sum(first))
        with torch.no_grad():
            q = self.model.forward_varlen(patches, pos, scales, first)[0]
        return mean_over_repeats(q, R)

    # ---- the two entries ----------------------------------------------------------------------------------------------------------
    def __call__(self, ref, dist, keys=None, aligned: bool = True) -> torch.Tensor:
        """B pairs.  ref, dist: float (B, 3, H, W) tensors -- float32, float16 or bfloat16, contiguous, used in place -- or lists of B
        (3, H_i, W_i) tensors (concatenated on the device: one copy); or device-resident uint8 (B, H, W, 3) tensors / lists of
        (H_i, W_i, 3).  keys: B 64-bit keys, one per pair (aligned=True: both images of a pair get its key and must have one size, so they
        get the same coordinates) or 2B, references first (aligned=False: two coordinate sets); None: from the call counter.
        Returns q (B,) fp32 on the device -- fp64 with num_repeats > 1.  Refused before anything is enqueued: CPU tensors (RuntimeError),
        float64 / integer pixels and two dtypes (TypeError), a strided or channels_last batch (ValueError naming .contiguous()), a pair of
        two sizes with aligned=True and an image smaller than a patch (ValueError), WeightedPatchSampler with float images
        (NotImplementedError: its integer pixel weight is defined on bytes; with uint8 images it is sampling.sample_patches_weighted)."""
        r, d = self._images(ref, dist, ("ref", "dist"))
        B = len(r.sizes)
        if len(d.sizes) != B:
            raise ValueError(f"ref and dist: B >= 1 images each ({B} and {len(d.sizes)} given)")
        if aligned:
            _aligned_sizes(r.sizes, d.sizes)
        kr, kd = pair_keys(keys, self.count, B, aligned)
        counts = patch_counts(self.patch_count, B)
        if isinstance(self.sampler, WeightedPatchSampler):
            return self._weighted(r, d, counts, kr, kd, aligned)
        sr = self._plan(r, counts, kr)
        sd = sr if aligned else self._plan(d, counts, kd)
        patches, pos, scales = self._patches(r, d, sr, sd, aligned)
        with torch.no_grad():
            q = self.model.forward_varlen(patches, pos, scales if scales[0] is not None else (None, None), sr.lengths)[0]
        return mean_over_repeats(q, self.num_repeats)

    def group(self, refs, dists, ref_index, keys=None, patch_count_dist=None) -> torch.Tensor:
        """G references and M distorted images of any sizes, image m scored against reference ref_index[m]; every reference is gathered and
        encoded once (forward_group(lengths=)).  The metric's patch_count is per reference (one int or G); patch_count_dist: one int or M
        (default: patch_count, which must then be one int).  keys: G + M keys, references first (None: from the call counter); a distorted
        image with its reference's key, size and count gets its reference's coordinates.  Returns q (M,), fp64 with num_repeats > 1."""
        r, d = self._images(refs, dists, ("refs", "dists"))
        G, M, R = len(r.sizes), len(d.sizes), self.num_repeats
        idx = _ref_indices(ref_index, G, M)
        if patch_count_dist is None:
            if np.ndim(self.patch_count) != 0:
                raise ValueError("patch_count per reference needs patch_count_dist for the distorted images")
            patch_count_dist = self.patch_count
        k = as_keys(default_keys(self.count, G + M) if keys is None else keys, G + M)
        sr, sd = self._plan(r, patch_counts(self.patch_count, G), k[:G]), self._plan(d, patch_counts(patch_count_dist, M), k[G:])
        patches, pos, scales = self._patches(r, d, sr, sd, False)
        with torch.no_grad():
            q = self.model.forward_group(patches, pos, scales if scales[0] is not None else (None, None),
                                         [i + rep * G for rep in range(R) for i in idx], lengths=(sr.lengths, sd.lengths))[0]
        return mean_over_repeats(q, R)
