"""Host images in, scores out: the loader side of a validation / test pass, pipelined (SURVEY.md 8f-1 + 8f-4).

The reference's loader builds the fp32 patch tensor on the CPU (data/patch_datasets.py:397-409, data/patch_sampling.py:529-611) and ships
3.08 MB per pair to the GPU; here the CPU only SAMPLES patch coordinates (RNG parity is not required) and the uint8 images themselves cross
PCIe (1.19 MB per pair at 384 x 512): pinned host buffers -> H2D on a copy stream -> patches.extract_patches (normalise, pyramid, gather on
the GPU) -> the model's forward, with `depth` buffer sets so that the copy of batch i + 1 runs under the forward of batch i.  Scores stay on
the device (validate.compute_correlations_cat_flat reduces them there).

    pipe = ImagePairPipeline(model, pairs_per_batch=32, image_hw=(384, 512), patches=500)
    for i, (ref_u8, dist_u8, samples) in enumerate(loader):          # numpy / torch uint8 [B, H, W, 3] each, int32 [B, N, 2] (aligned) or [2B, N, 2]
        q = pipe.submit(ref_u8, dist_u8, samples)                     # device tensor [B]; returns as soon as the work is enqueued
        scores.append(q)
    # or, without the host copy: img, smp, sid = pipe.acquire(); <decode into the pinned views>; q = pipe.launch()

Measured (bench.py `e2e`, profiles/r05_bench_line.json): the loop sustains 0.98 x the forward's own throughput at B = 32, N = 500; with a 1 280-pair
validation set's final reductions (rank statistics + the logistic fit, once per set) 0.91 - 0.95 x by box.

Batches that mix image sizes and patch counts go through ImagePairVarlenPipeline below: one gather over all images of the batch
(patches.gather_patches_u8) and forward_varlen / forward_group(lengths=), 0.977 x of forward_varlen alone (profiles/r15_image_varlen.txt).
Its submit_images / submit_group_images take the images alone: the coordinates are sampled on the device (sampling.py,
include/vtamiq_hip_sampler.h; profiles/r16_sampler.txt).

Both pipelines are a _SlotRing, whose free_slot / upload / release ARE the slot protocol: no other code touches the copy stream or the
events.  The uniform pipeline's slot is three tensors of one shape; the varlen pipeline's is a byte arena and one int32 block whose word
ranges block_layout names for both kinds of batch (VarlenBatch: host-sampled, SampledBatch: device-sampled).  Every varlen entry is
plan -> _stage (the one place a slot's host side is written) -> _upload_and_gather (the one place it is enqueued; the sampler is its
optional step on the copy stream) -> _as_pairs or _as_group.  The argument checks the entries share stand in front of the classes.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .patches import ImageTables, check_samples_host, check_samples_host_varlen, extract_patches, gather_patches_u8, image_tables, table_rows
from .sampling import (DEFAULT_NUM_SAMPLES_RATIO, MAX_CELLS, PatchSampler, WeightedPatchSampler, as_keys, launch_diff_cells, launch_sample_grid,
                       launch_sample_weighted, patch_counts, plan_samples, plan_samples_weighted, repeat_key, segments_for)


class _SlotRing:
    """`depth` buffer sets (slots) used in turn, a copy stream and two events per slot.  The protocol of a submission on slot s:
      free_slot()   the host waits for consumed[s]: the batch `depth` submissions ago no longer reads the slot's host or device buffers
      upload()      on the copy stream: wait for consumed[s], the H2D copies, an optional step behind them, record copied[s]; the stream
                    current at the call then waits for copied[s]
      release()     record consumed[s] on the current stream, directly behind the gather that read the slot -- not behind the forward
    `count` is the number of submissions enqueued; a refused batch is not counted and enqueues nothing."""

    def __init__(self, device: Optional[torch.device], depth: int):
        if depth < 2:
            raise ValueError("depth >= 2 (one buffer set is being filled while another is consumed)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (no CPU fallback on the product path)")
        self.depth = depth
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.copied = [torch.cuda.Event() for _ in range(depth)]
        self.consumed = [torch.cuda.Event() for _ in range(depth)]
        main = torch.cuda.current_stream(self.device)
        for ev in self.consumed:
            ev.record(main)
        self.count = 0

    def free_slot(self) -> int:
        s = self.count % self.depth
        self.consumed[s].synchronize()
        return s

    def upload(self, s: int, copies, behind=None) -> None:
        """copies: (device tensor, pinned host tensor) pairs; behind: run with the copy stream current.  Counts the submission."""
        self.count += 1
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(self.consumed[s])    # the slot's device buffers were read by batch i - depth
            for dst, src in copies:
                dst.copy_(src, non_blocking=True)
            if behind is not None:
                behind()
            self.copied[s].record(self.copy_stream)
        main.wait_event(self.copied[s])

    def release(self, s: int) -> None:
        self.consumed[s].record(torch.cuda.current_stream(self.device))


# ---- argument checks shared by the entries, device-free ------------------------------------------------------------------------------------
def _two_sides(x, B: int, what: str):
    """x for B pairs, shared by a pair's two images (aligned sampling), or for 2B images, references first -> (first side's, second's)."""
    if len(x) not in (B, 2 * B):
        raise ValueError(f"{what}: B (aligned, shared by a pair's two images) or 2B (references first), B = {B}")
    return (x, x) if len(x) == B else (x[:B], x[B:])


def _host_images(refs, dists, pairs: bool = False):
    """Two lists of host images uint8 [H, W, 3] as numpy arrays, at least one each; pairs: as many distorted images as references."""
    refs, dists = [np.asarray(r) for r in refs], [np.asarray(d) for d in dists]
    if len(refs) < 1 or len(dists) < 1 or (pairs and len(dists) != len(refs)):
        raise ValueError("refs and dists: B >= 1 images each" if pairs else "refs and dists: at least one image each")
    if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in refs + dists):
        raise ValueError("images must be uint8 [H, W, 3]")
    return refs, dists


def _aligned_sizes(sizes_ref, sizes_dist) -> None:
    """Aligned sampling gives a pair's two images the same coordinates: their (H, W) must be equal."""
    for b, (r, d) in enumerate(zip(sizes_ref, sizes_dist)):
        if tuple(r) != tuple(d):
            raise ValueError(f"aligned sampling: pair {b}'s images differ in size ({tuple(r)}, {tuple(d)}); pass 2B sample arrays / aligned=False")


def default_keys(count: int, n: int) -> list:
    """keys=None: image / pair b of a caller's i-th submission (count = i) gets (i << 32) | b."""
    return [(count << 32) | b for b in range(n)]


def pair_keys(keys, count: int, B: int, aligned: bool):
    """(reference keys, distorted keys) of B pairs as uint64: B keys, one per pair (aligned: both images get the pair's key), or 2B,
    references first; None: from the submission counter, the distorted image's with the top bit flipped when unaligned."""
    if aligned:
        k = as_keys(default_keys(count, B) if keys is None else keys, B)
        return k, k
    k2 = as_keys(keys, 2 * B) if keys is not None else as_keys([k ^ (s << 63) for s in (0, 1) for k in default_keys(count, B)], 2 * B)
    return k2[:B], k2[B:]


def repeat_keys(keys: np.ndarray, repeats: int) -> np.ndarray:
    """The keys of `repeats` validation repeats, repeat-major: sampling.repeat_key(key, r) for r = 0 .. repeats - 1."""
    return np.array([repeat_key(k, r) for r in range(repeats) for k in keys.tolist()], dtype=np.uint64)


def mean_over_repeats(q: torch.Tensor, repeats: int) -> torch.Tensor:
    """Repeat-major scores (repeats * n,) -> their mean over the repeats on the device (fp64 (n,)); q itself for one repeat."""
    if repeats == 1:
        return q
    from .validate import average_over_repeats
    return average_over_repeats(q, repeats)


def _ref_indices(ref_index, G: int, M: int) -> list:
    idx = [int(i) for i in ref_index]
    if len(idx) != M or any(not 0 <= i < G for i in idx):
        raise ValueError("ref_index: one reference in [0, G) per distorted image")
    return idx


def _sample_lists(samples, scale_ids, num_scales: int):
    """One integer array (N_i, 2), N_i >= 1, per image and, with levels, one scale-id array (N_i,) each -> (samples, scale ids or None)."""
    smp = [np.asarray(s) for s in samples]
    if any(s.ndim != 2 or s.shape[1] != 2 or s.shape[0] < 1 or s.dtype.kind not in "iu" for s in smp):
        raise ValueError("samples: integer arrays (N, 2), N >= 1")
    if num_scales <= 1:
        return smp, None
    if scale_ids is None:
        raise ValueError("scale_ids are required when num_scales > 1")
    sid = [np.asarray(i) for i in scale_ids]
    if len(sid) != len(smp) or any(i.shape != (s.shape[0],) for i, s in zip(sid, smp)):
        raise ValueError("scale_ids: one array (N,) per sample array")
    return smp, sid


def _sides(out, k: int):
    """The gather's (patches, pos, scales) split behind row k: the call tensors of the two sides."""
    patches, pos, scales = out
    return (patches[:k], patches[k:]), (pos[:k], pos[k:]), ((scales[:k], scales[k:]) if scales is not None else (None, None))


class ImagePairPipeline(_SlotRing):
    def __init__(self, model, pairs_per_batch: int, image_hw: Tuple[int, int], patches: int, num_scales: int = 1,
                 device: Optional[torch.device] = None, depth: int = 2, mean: Sequence[float] = (0.5, 0.5, 0.5),
                 std: Sequence[float] = (0.5, 0.5, 0.5)):
        super().__init__(device, depth)
        self.model = model
        self.B, self.N, self.num_scales = int(pairs_per_batch), int(patches), int(num_scales)
        self.H, self.W, self.P = int(image_hw[0]), int(image_hw[1]), model.spec.patch_size
        self.mean, self.std = tuple(mean), tuple(std)
        NI = 2 * self.B
        self.host_img = [torch.empty(NI, self.H, self.W, 3, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.host_smp = [torch.empty(NI, self.N, 2, dtype=torch.int32).pin_memory() for _ in range(depth)]
        self.host_sid = [torch.zeros(NI, self.N, dtype=torch.int32).pin_memory() for _ in range(depth)] if num_scales > 1 else None
        self.dev_img = [torch.empty(NI, self.H, self.W, 3, dtype=torch.uint8, device=self.device) for _ in range(depth)]
        self.dev_smp = [torch.empty(NI, self.N, 2, dtype=torch.int32, device=self.device) for _ in range(depth)]
        self.dev_sid = [torch.empty(NI, self.N, dtype=torch.int32, device=self.device) for _ in range(depth)] if num_scales > 1 else None

    @staticmethod
    def _np(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    def acquire(self):
        """The next slot's PINNED host buffers as numpy views -- images uint8 [2B, H, W, 3] (ref rows first), samples int32 [2B, N, 2], scale ids
        int32 [2B, N] or None -- once the batch that used them `depth` submissions ago no longer reads them.  A loader that decodes straight
        into these views saves the host copy of submit(); follow with launch()."""
        s = self.free_slot()
        return self.host_img[s].numpy(), self.host_smp[s].numpy(), (self.host_sid[s].numpy() if self.host_sid is not None else None)

    def launch(self) -> torch.Tensor:
        """Enqueue the slot filled through acquire(): range check of the samples on the host, H2D on the copy stream, gather + forward on the
        current stream.  Returns the batch's scores as a device tensor [B]."""
        s, B, multi = self.count % self.depth, self.B, self.host_sid is not None
        # the range check the reference gets from numpy fancy-indexing, on the host copy (no GPU synchronisation, no torch CPU operators)
        check_samples_host(self.host_smp[s], self.host_sid[s] if multi else None, self.H, self.W, self.num_scales, self.P)
        self.upload(s, [(self.dev_img[s], self.host_img[s]), (self.dev_smp[s], self.host_smp[s])]
                    + ([(self.dev_sid[s], self.host_sid[s])] if multi else []))
        out = extract_patches(self.dev_img[s], self.dev_smp[s], self.dev_sid[s] if multi else None, self.num_scales, mean=self.mean,
                              std=self.std, patch_size=self.P, validate=False)
        self.release(s)                                      # behind the gather: the uint8 images and the samples of the slot are free again
        with torch.no_grad():
            return self.model(*_sides(out, B))[0]

    def submit(self, ref_u8, dist_u8, samples, scale_ids=None) -> torch.Tensor:
        """One batch of B pairs: ref / dist uint8 images [B, H, W, 3] (host), sampled patch coordinates int32 [B, N, 2] (shared by ref and
        dist: aligned sampling, the reference's default) or [2B, N, 2] (ref rows first), scale ids [B, N] / [2B, N] when num_scales > 1.
        Returns the batch's scores as a device tensor [B]; everything is enqueued asynchronously."""
        if self.host_sid is not None and scale_ids is None:
            raise ValueError("scale_ids are required when num_scales > 1")
        B, (img, hs, hd) = self.B, self.acquire()
        img[:B], img[B:] = self._np(ref_u8), self._np(dist_u8)
        hs[:B], hs[B:] = _two_sides(self._np(samples), B, "samples")
        if hd is not None:
            hd[:B], hd[B:] = _two_sides(self._np(scale_ids), B, "scale_ids")
        return self.launch()


# ---- batches whose images differ in size and patch count -----------------------------------------------------------------------------------
class BlockLayout(NamedTuple):
    """The word ranges of one batch in a slot's int32 block, in block order (block_layout)."""
    tab: slice                # [NI, 4] the image table
    patch_img: slice          # [T] the image of every patch row
    seg: slice                # [NS, 8] the sampler's segment table, from a multiple of 4 words on; empty when the host samples
    keys: slice               # NS uint64 keys as int32 pairs; empty when the host samples
    samples: slice            # [T, 2]
    ids: slice                # [T] scale ids; empty with one scale
    uploaded: int             # the words that cross PCIe, from word 0: all of them when the host samples, up to the samples when the device does
    words: int                # the words the batch uses

    def split(self, block):
        """(tab, patch_img, seg [NS, 8], keys, samples [T, 2], scale ids or None): views of a slot's block, host tensor or device twin."""
        ids = block[self.ids] if self.ids.stop > self.ids.start else None
        return (block[self.tab], block[self.patch_img], block[self.seg].view((self.seg.stop - self.seg.start) // 8, 8), block[self.keys],
                block[self.samples].view(self.patch_img.stop - self.patch_img.start, 2), ids)


def block_layout(n_images: int, n_patches: int, n_segments: Optional[int] = None, multi: bool = False) -> BlockLayout:
    """THE layout of a slot's int32 block, device-free, for NI table rows and T patch rows in all.  n_segments None, the host samples:
    tab | patch_img | samples | scale ids, all uploaded.  n_segments = NS, the device samples: tab | patch_img | (pad to 4 words) seg |
    keys, uploaded, then samples | scale ids, which the sampler writes and which never exist on the host."""
    a, b = 4 * n_images, 4 * n_images + n_patches
    seg_at = b if n_segments is None else (b + 3) // 4 * 4
    keys_at = seg_at + 8 * (n_segments or 0)
    front = keys_at + 2 * (n_segments or 0)
    c, d = front + 2 * n_patches, front + (3 if multi else 2) * n_patches
    return BlockLayout(slice(0, a), slice(a, b), slice(seg_at, keys_at), slice(keys_at, front), slice(front, c), slice(c, d),
                       d if n_segments is None else front, d)


def block_capacity(max_images: int, max_patches: int, num_scales: int) -> int:
    """int32 words of a slot's block: the largest layout a batch within max_images table rows, max_patches patches a side and num_scales
    levels (one segment per image and level at most) can have, of either kind, and one 16-byte unit of slack -- with it the block is
    never smaller than 4 max_images + 2 max_patches (4 | 3) + 10 num_scales max_images + 4, the size slots have always had."""
    return max(block_layout(max_images, 2 * max_patches, ns, num_scales > 1).words for ns in (None, num_scales * max_images)) + 4


class VarlenBatch(NamedTuple):
    """One batch as the varlen pipeline sees it, made on the host without a device (plan_varlen_batch)."""
    sizes: list               # NI (H, W): the first side's images, then the second side's
    lengths: np.ndarray       # int64 [NI] patches per image
    n_first: int              # images of the first side (references)
    tables: ImageTables
    words: int                # int32 words of the slot's table block this batch uses: tab, patch_img, samples, scale ids


def plan_varlen_batch(sizes_first, sizes_second, lengths_first, lengths_second, *, max_images: int, max_image_bytes: int, max_patches: int,
                      num_scales: int = 1, patch_size: int = 16) -> VarlenBatch:
    """Argument and capacity checking of ImagePairVarlenPipeline, device-free: the images of the first side (references) with their patch
    counts, then those of the second.  ValueError for a batch over capacity (max_images in all, max_image_bytes in all, max_patches per
    side), for an empty side or image, and for an image smaller than a patch."""
    sizes = [(int(h), int(w)) for h, w in list(sizes_first) + list(sizes_second)]
    lf, ls = np.asarray(lengths_first, dtype=np.int64).reshape(-1), np.asarray(lengths_second, dtype=np.int64).reshape(-1)
    if len(sizes_first) < 1 or len(sizes_second) < 1 or len(lf) != len(sizes_first) or len(ls) != len(sizes_second):
        raise ValueError("each side needs at least one image and one patch count per image")
    if (lf < 1).any() or (ls < 1).any():
        raise ValueError("every image needs at least one patch")
    if len(sizes) > max_images:
        raise ValueError(f"{len(sizes)} images in the batch, the pipeline was built for {max_images} (2 * max_pairs)")
    if max(int(lf.sum()), int(ls.sum())) > max_patches:
        raise ValueError(f"{max(int(lf.sum()), int(ls.sum()))} patches on one side, the pipeline was built for max_patches={max_patches}")
    lengths = np.concatenate([lf, ls])
    tables = image_tables(sizes, lengths)
    if tables.image_bytes > max_image_bytes:
        raise ValueError(f"the batch's images take {tables.image_bytes} bytes, the pipeline was built for max_image_bytes={max_image_bytes}")
    P = int(patch_size)
    for i, (h, w) in enumerate(sizes):
        if h < P or w < P:
            raise ValueError(f"image {i} ({h}x{w}) is smaller than one {P}x{P} patch")
    return VarlenBatch(sizes, lengths, len(sizes_first), tables, block_layout(len(sizes), tables.total, None, num_scales > 1).words)


def pair_arguments(refs, dists, samples, lengths=None, scale_ids=None, num_scales: int = 1):
    """submit()'s argument checking, device-free.  refs, dists: B host images uint8 [H, W, 3] each; samples: B arrays (N_b, 2) -- aligned
    sampling, one list per pair shared by its two images, which must then have ONE size -- or 2B arrays (references first) for unaligned
    sampling with N_b patches on both sides of pair b; lengths: None or the B counts, which must then match; scale_ids like samples.
    Returns (refs, dists, per-image samples [2B], per-image scale ids [2B] or None, lengths [B]) as numpy arrays."""
    refs, dists = _host_images(refs, dists, pairs=True)
    B = len(refs)
    first, second = _two_sides(list(samples), B, "samples")
    if first is second:
        _aligned_sizes([r.shape[:2] for r in refs], [d.shape[:2] for d in dists])
    ids = None
    if scale_ids is not None and num_scales > 1:
        ids_first, ids_second = _two_sides(list(scale_ids), B, "scale_ids")
        ids = ids_first + ids_second
    smp, sid = _sample_lists(first + second, ids, num_scales)
    lens = [s.shape[0] for s in smp[:B]]
    if [s.shape[0] for s in smp[B:]] != lens:
        raise ValueError("the two images of a pair need the same patch count")
    if lengths is not None and [int(n) for n in lengths] != lens:
        raise ValueError("lengths do not match the sample arrays")
    return refs, dists, smp, sid, lens


class SampledBatch(NamedTuple):
    """One batch whose coordinates the device samples (plan_sampled_batch): the varlen batch over its R-fold image list, whose table rows
    of repeat r > 0 point at the bytes of repeat 0, and the sampler's segment table and keys."""
    batch: VarlenBatch        # sizes / lengths / tables of the R * NI table rows, first side first, repeat-major within a side
    seg: np.ndarray           # int32 [NS, 8]  sampling.plan_samples over those rows
    seg_keys: np.ndarray      # uint64 [NS]
    n_images: int             # NI: the images that cross PCIe (rows 0 .. of each side's repeat 0)
    repeats: int
    front: int                # int32 words of the slot's block that are uploaded: tab, patch_img, seg, keys
    seg_at: int               # word offset of seg in the block (a multiple of 4); the keys follow it, the device-only samples and ids those


def plan_sampled_batch(sizes_first, sizes_second, counts_first, counts_second, keys_first, keys_second, *, max_images: int,
                       max_image_bytes: int, max_patches: int, repeats: int = 1, num_scales: int = 1,
                       scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO, patch_size: int = 16) -> SampledBatch:
    """Argument and capacity checking of submit_images / submit_group_images, device-free.  Each side's images appear `repeats` times,
    repeat-major, with the keys sampling.repeat_key(key, r): repeats count against max_images and max_patches, the image bytes once.
    ValueError as plan_varlen_batch, before anything is written."""
    R = int(repeats)
    if R < 1:
        raise ValueError("num_repeats >= 1")
    nf, ns_ = len(sizes_first), len(sizes_second)
    base = plan_varlen_batch(sizes_first, sizes_second, counts_first, counts_second, max_images=max_images, max_image_bytes=max_image_bytes,
                             max_patches=max_patches, num_scales=num_scales, patch_size=patch_size)
    if R * len(base.sizes) > max_images:
        raise ValueError(f"{R * len(base.sizes)} images in the batch ({R} repeats), the pipeline was built for {max_images} (2 * max_pairs)")
    side = R * max(int(base.lengths[:nf].sum()), int(base.lengths[nf:].sum()))
    if side > max_patches:
        raise ValueError(f"{side} patches on one side ({R} repeats), the pipeline was built for max_patches={max_patches}")
    kf, ks = as_keys(keys_first, nf), as_keys(keys_second, ns_)
    rows = np.concatenate([np.tile(np.arange(nf), R), np.tile(np.arange(nf, nf + ns_), R)])          # the base image of every table row
    keys = np.concatenate([repeat_keys(kf, R), repeat_keys(ks, R)])
    sizes = [base.sizes[i] for i in rows]
    lengths = base.lengths[rows]
    plan = plan_samples(sizes, lengths.tolist(), num_scales, scale_num_samples_ratio, patch_size)
    t = base.tables
    tables = table_rows(t, rows, lengths)
    layout = block_layout(len(rows), tables.total, len(plan.seg), num_scales > 1)
    batch = VarlenBatch(sizes, lengths, R * nf, tables, layout.words)
    return SampledBatch(batch, np.ascontiguousarray(plan.seg), np.ascontiguousarray(keys[plan.seg_image]), nf + ns_, R, layout.uploaded,
                        layout.seg.start)


class ImagePairVarlenPipeline(_SlotRing):
    """ImagePairPipeline for batches whose images differ in size and patch count: host uint8 images in, scores out, through ONE gather over
    all images of the batch (patches.extract_patches_varlen's kernel) and forward_varlen -- or, one reference against many distorted images,
    forward_group(lengths=).  Slots are sized by capacity, not by shape:

        pipe = ImagePairVarlenPipeline(model, max_pairs=32, max_image_bytes=2 * 32 * 3 * 512 * 512, max_patches=32 * 600)
        q = pipe.submit(refs, dists, samples)               # lists of B host images and B (N_b, 2) sample arrays; q (B,) on the device
        q = pipe.submit_group(refs, dists, ref_index, samples_ref, samples_dist)
        q = pipe.submit_images(refs, dists, 500, keys=pair_ids)     # no coordinates: sampled on the device (sampling.py); likewise
        q = pipe.submit_group_images(refs, dists, ref_index, 500)   # the one-to-many form; num_repeats=R averages R samplings per pair

    Each of the `depth` slots owns one pinned byte arena for the images and one pinned int32 block for the tables, samples and scale ids, and
    their device twins: a batch is two H2D copies on the copy stream, none from pageable memory, and nothing synchronises but the wait for
    the slot's previous batch (`consumed`).  A loader that decodes straight into the pinned views uses acquire() / launch()."""

    def __init__(self, model, max_pairs: int, max_image_bytes: int, max_patches: int, num_scales: int = 1,
                 device: Optional[torch.device] = None, depth: int = 2, mean: Sequence[float] = (0.5, 0.5, 0.5),
                 std: Sequence[float] = (0.5, 0.5, 0.5)):
        if max_pairs < 1 or max_image_bytes < 1 or max_patches < 1:
            raise ValueError("max_pairs, max_image_bytes and max_patches must be positive")
        super().__init__(device, depth)
        self.model = model
        self.max_images, self.max_image_bytes, self.max_patches = 2 * int(max_pairs), int(max_image_bytes), int(max_patches)
        self.num_scales, self.P = int(num_scales), model.spec.patch_size
        self.mean, self.std = tuple(mean), tuple(std)
        self._caps = dict(max_images=self.max_images, max_image_bytes=self.max_image_bytes, max_patches=self.max_patches,
                          num_scales=self.num_scales, patch_size=self.P)
        words = block_capacity(self.max_images, self.max_patches, self.num_scales)
        self.host_img = [torch.empty(self.max_image_bytes, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.host_tab = [torch.zeros(words, dtype=torch.int32).pin_memory() for _ in range(depth)]
        self.dev_img = [torch.empty(self.max_image_bytes, dtype=torch.uint8, device=self.device) for _ in range(depth)]
        self.dev_tab = [torch.empty(words, dtype=torch.int32, device=self.device) for _ in range(depth)]
        self._batch = None
        self._weighted = None                                # the weighted sampler's per-slot tables, made when it is first asked for

    def plan(self, sizes_first, sizes_second, lengths_first, lengths_second) -> VarlenBatch:
        return plan_varlen_batch(sizes_first, sizes_second, lengths_first, lengths_second, **self._caps)

    # ---- one path for every entry: stage the slot's host side, upload it and gather, end as pairs or as a group -----------------------
    def _layout(self, planned):
        """(the VarlenBatch, its block_layout) of a planned batch, VarlenBatch or SampledBatch."""
        batch, ns = (planned.batch, len(planned.seg)) if isinstance(planned, SampledBatch) else (planned, None)
        return batch, block_layout(len(batch.sizes), batch.tables.total, ns, self.num_scales > 1)

    def _stage(self, planned):
        """The one place a slot's host side is written: wait for the next slot, write the batch's tables (a SampledBatch's segment table
        and keys with them) into its pinned block, and return numpy views of what the caller fills -- the images that cross PCIe in the
        pinned arena, uint8 [H_i, W_i, 3] each, the samples int32 (total, 2) and the scale ids int32 (total,) or None."""
        s = self.free_slot()
        sb = planned if isinstance(planned, SampledBatch) else None
        batch, layout = self._layout(planned)
        t = batch.tables
        tab, pimg, seg, keys, smp, sid = layout.split(self.host_tab[s])
        tab.numpy()[:] = t.tab.reshape(-1)
        pimg.numpy()[:] = t.patch_img
        rows = range(len(batch.sizes))
        if sb is not None:
            seg.numpy()[:] = sb.seg
            keys.numpy()[:] = sb.seg_keys.view(np.int32)
            nf = batch.n_first // sb.repeats                 # the table rows of repeat 0 of each side: the images that are copied
            rows = list(range(nf)) + list(range(batch.n_first, batch.n_first + sb.n_images - nf))
        arena, off = self.host_img[s].numpy(), t.img_off.tolist()
        views = [arena[off[i]:off[i] + 3 * h * w].reshape(h, w, 3) for i in rows for h, w in [batch.sizes[i]]]
        return views, smp.numpy(), (sid.numpy() if sid is not None else None)

    def _upload_and_gather(self, planned, behind=None):
        """The one place a staged slot is enqueued: two H2D copies on the copy stream (the arena's used bytes, the block's uploaded
        words) and behind them `behind(seg, keys, samples, scale_ids)` on the slot's device block, then on the current stream the gather,
        with `consumed` directly behind it.  Returns the gather's (patches, pos, scales)."""
        s, (batch, layout) = self.count % self.depth, self._layout(planned)
        t = batch.tables
        dtab, dpimg, dseg, dkeys, dsmp, dsid = layout.split(self.dev_tab[s])
        self._batch = None
        self.upload(s, [(self.dev_img[s][:t.image_bytes], self.host_img[s][:t.image_bytes]),
                        (self.dev_tab[s][:layout.uploaded], self.host_tab[s][:layout.uploaded])],
                    (lambda: behind(dseg, dkeys, dsmp, dsid)) if behind is not None else None)
        out = gather_patches_u8(self.dev_img[s][:t.image_bytes], t, dtab, dpimg, dsmp, dsid, None, self.num_scales, self.mean, self.std, self.P)
        self.release(s)                                      # behind the gather: the slot's images, tables and samples are free again
        return out

    def _as_pairs(self, batch: VarlenBatch, out) -> torch.Tensor:
        first = batch.lengths[:batch.n_first]
        with torch.no_grad():
            return self.model.forward_varlen(*_sides(out, int(first.sum())), first.tolist())[0]

    def _as_group(self, batch: VarlenBatch, out, index) -> torch.Tensor:
        L, G = batch.lengths, batch.n_first
        with torch.no_grad():
            return self.model.forward_group(*_sides(out, int(L[:G].sum())), index, lengths=(L[:G].tolist(), L[G:].tolist()))[0]

    def acquire(self, batch: VarlenBatch):
        """The next slot's PINNED host buffers for `batch` (plan()) as numpy views, once the batch that used the slot `depth` submissions
        ago no longer reads it: a list of the NI images uint8 [H_i, W_i, 3] (first side first), samples int32 (total, 2) and scale ids
        int32 (total,) or None, both concatenated in image order.  The tables are written here.  Follow with launch() or launch_group()."""
        pinned = self._stage(batch)
        self._batch = batch
        return pinned

    def _launch(self, validate: bool):
        batch = self._batch
        if batch is None:
            raise RuntimeError("launch() without acquire()")
        if validate:
            # the range check the reference gets from numpy fancy-indexing, on the host copy: before anything is enqueued
            *_, smp, sid = self._layout(batch)[1].split(self.host_tab[self.count % self.depth])
            check_samples_host_varlen(smp.numpy(), sid.numpy() if sid is not None else None, batch.sizes, batch.lengths, self.num_scales,
                                      self.P)
        return batch, self._upload_and_gather(batch)

    def launch(self, validate: bool = True) -> torch.Tensor:
        """Enqueue the slot filled through acquire() as B pairs (image b of the first side with image b of the second, equal patch counts):
        range check on the host, two H2D copies on the copy stream, gather + forward_varlen on the current stream.  Returns q (B,)."""
        b = self._batch
        if b is not None and (2 * b.n_first != len(b.sizes) or not np.array_equal(b.lengths[:b.n_first], b.lengths[b.n_first:])):
            raise ValueError("pairs need as many second-side images as first-side ones, with the same patch counts")
        return self._as_pairs(*self._launch(validate))

    def launch_group(self, ref_index, validate: bool = True) -> torch.Tensor:
        """Enqueue the slot filled through acquire() as G references (first side) and M distorted images (second side) with
        ref_index[m] in [0, G): ends in forward_group(..., ref_index, lengths=(lengths_ref, lengths_dist)).  Returns q (M,)."""
        b = self._batch
        idx = _ref_indices(ref_index, b.n_first, len(b.sizes) - b.n_first) if b is not None else None
        return self._as_group(*self._launch(validate), idx)

    def _fill(self, batch, images, smp, sid):
        smp, sid = np.concatenate(smp), (np.concatenate(sid) if sid is not None else None)
        # checked on the caller's arrays, so that a refused batch leaves the slot and the streams alone
        check_samples_host_varlen(smp, sid, batch.sizes, batch.lengths, self.num_scales, self.P)
        views, hs, hd = self.acquire(batch)
        for v, im in zip(views, images):
            v[...] = im
        hs[:] = smp
        if hd is not None:
            hd[:] = sid

    def submit(self, refs, dists, samples, lengths=None, scale_ids=None) -> torch.Tensor:
        """One batch of B pairs of any sizes: refs / dists lists of B host images uint8 [H, W, 3]; samples B arrays (N_b, 2) shared by a
        pair's two images (aligned sampling: the two must have one size, else ValueError) or 2B arrays, references first (unaligned);
        scale_ids likewise, (N_b,), when num_scales > 1.  ValueError for a batch over the slot capacity and IndexError for a sample
        outside its image's level, both before anything is enqueued.  Returns q (B,) on the device; everything is asynchronous."""
        refs, dists, smp, sid, lens = pair_arguments(refs, dists, samples, lengths, scale_ids, self.num_scales)
        batch = self.plan([r.shape[:2] for r in refs], [d.shape[:2] for d in dists], lens, lens)
        self._fill(batch, refs + dists, smp, sid)
        return self.launch(validate=False)

    def submit_group(self, refs, dists, ref_index, samples_ref, samples_dist, scale_ids_ref=None, scale_ids_dist=None) -> torch.Tensor:
        """G reference images and M distorted ones of any sizes and patch counts, distorted image m scored against reference ref_index[m]:
        every reference crosses PCIe once and is encoded once.  samples_ref: G arrays (N_g, 2), samples_dist: M arrays (N_m, 2); scale ids
        likewise when num_scales > 1.  Returns q (M,) on the device."""
        refs, dists = _host_images(refs, dists)
        G = len(refs)
        if len(samples_ref) != G or len(samples_dist) != len(dists):
            raise ValueError("one sample array per image")
        ids = None if scale_ids_ref is None or scale_ids_dist is None else list(scale_ids_ref) + list(scale_ids_dist)
        smp, sid = _sample_lists(list(samples_ref) + list(samples_dist), ids, self.num_scales)
        batch = self.plan([r.shape[:2] for r in refs], [d.shape[:2] for d in dists], [s.shape[0] for s in smp[:G]], [s.shape[0] for s in smp[G:]])
        idx = _ref_indices(ref_index, G, len(dists))
        self._fill(batch, refs + dists, smp, sid)
        return self.launch_group(idx, validate=False)

    # ---- coordinates sampled on the device (sampling.py, include/vtamiq_hip_sampler.h) ----------------------------------------------
    def plan_sampled(self, sizes_first, sizes_second, counts_first, counts_second, keys_first, keys_second, repeats: int = 1,
                     scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO) -> SampledBatch:
        return plan_sampled_batch(sizes_first, sizes_second, counts_first, counts_second, keys_first, keys_second, repeats=repeats,
                                  scale_num_samples_ratio=scale_num_samples_ratio, **self._caps)

    def _sample_and_gather(self, sb: SampledBatch, images, seed: int, sampler: Optional[PatchSampler]):
        """Stage the batch's images and tables and, as the upload's step on the copy stream, launch the sampler into the slot's device
        block: behind the tables it reads and under the forward of the batch before, not in front of this batch's gather on the current
        stream (the slot's samples were last read by batch i - depth: `consumed`).  The coordinates never exist on the host."""
        sampler = sampler if sampler is not None else PatchSampler()
        views, _, _ = self._stage(sb)
        for v, im in zip(views, images):
            v[...] = im
        return self._upload_and_gather(sb, lambda seg, keys, smp, sid: launch_sample_grid(seg, keys, sb.seg, sb.seg_keys, seed,
                                                                                          sampler.amount_q, smp, sid))

    def _weighted_slots(self):
        """Per slot, sized by capacity: a pinned int32 block and its device twin for the weighted sampler's segment table, keys, pair and
        level tables, and the device's uint64 weight table (4 words per pair, 2 + 8192 per pair and level at most)."""
        if self._weighted is None:
            ns, pairs = self.num_scales * self.max_images, self.max_images // 2
            words = 14 * ns + 16 * pairs + 8 * self.num_scales * pairs + 4
            sums = pairs * (4 + self.num_scales * (2 + MAX_CELLS))
            self._weighted = ([torch.zeros(words, dtype=torch.int32).pin_memory() for _ in range(self.depth)],
                              [torch.empty(words, dtype=torch.int32, device=self.device) for _ in range(self.depth)],
                              [torch.empty(sums, dtype=torch.int64, device=self.device) for _ in range(self.depth)])
        return self._weighted

    def _sample_weighted_and_gather(self, sb: SampledBatch, images, seed: int, sampler: WeightedPatchSampler, ratio: float):
        """_sample_and_gather with the weighted sampler: the pair, level and segment tables go up in one more copy on the copy stream, and
        behind the images the difference pass runs ONCE per pair -- whatever the number of repeats, and for both images of the pair,
        aligned or not -- followed by one sampler launch over every segment of the batch.  With diff_weight == 0 no pixel is read.
        Everything the two entries refuse is refused here first, by plan_samples_weighted and the sampler's constructor, before the slot
        is staged: the tables the entries see are this function's own."""
        B, R = len(images) // 2, sb.repeats
        base = sb.batch.tables.img_off
        plan = plan_samples_weighted(sb.batch.sizes, sb.batch.lengths.tolist(), self.num_scales, ratio, self.P,
                                     pair_of=[i % B for i in range(len(sb.batch.sizes))])
        if plan.seg.shape[0] != sb.seg.shape[0] or not np.array_equal(plan.seg[:, :2], sb.seg[:, :2]):
            raise RuntimeError("the weighted plan's segments are not those of the batch's plan (rows, counts per level)")
        pairs = plan.pairs.copy()
        pairs[:, 0], pairs[:, 1] = base[:B], base[R * B:R * B + B]
        NS, NL = plan.seg.shape[0], plan.lev.shape[0]
        seg, lev = segments_for(plan, sampler), np.ascontiguousarray(plan.lev)
        host, dev, sums = self._weighted_slots()
        views, _, _ = self._stage(sb)
        for v, im in zip(views, images):
            v[...] = im
        s = self.count % self.depth
        at = np.cumsum([0, 12 * NS, 2 * NS + (-2 * NS) % 4, 16 * B, 8 * NL])
        h = host[s].numpy()
        h[at[0]:at[1]], h[at[1]:at[1] + 2 * NS] = seg.reshape(-1), sb.seg_keys.view(np.int32)
        h[at[2]:at[3]], h[at[3]:at[4]] = pairs.reshape(-1).view(np.int32), plan.lev.reshape(-1)
        flat, d, tab = self.dev_img[s][:sb.batch.tables.image_bytes], dev[s], sums[s]
        weigh = sampler.diff_weight > 0

        def behind(_seg, _keys, smp, sid):
            d[:at[4]].copy_(host[s][:at[4]], non_blocking=True)
            if weigh:
                launch_diff_cells(flat, d[at[2]:at[3]], d[at[3]:at[4]], pairs, lev, self.P, tab, plan.tab_words)
            launch_sample_weighted(d[at[0]:at[1]], d[at[1]:at[1] + 2 * NS], seg, sb.seg_keys, self.P, tab if weigh else None,
                                   plan.tab_words if weigh else 0, sampler, seed, smp, sid)

        return self._upload_and_gather(sb, behind)

    def submit_images(self, refs, dists, patch_count, keys=None, seed: int = 0, aligned: bool = True, num_repeats: int = 1,
                      sampler: Optional[PatchSampler] = None, scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO) -> torch.Tensor:
        """submit() without coordinates: B pairs of host images uint8 [H, W, 3] and patch_count patches per image (one int, or B), sampled
        on the device by the reference's default sampler (sampling.py) -- or, with sampler=WeightedPatchSampler(diff_weight, uniform_weight),
        where the pair's images differ: the difference pass and the weighted sampler run on the copy stream behind the upload, once and R
        times for num_repeats=R, and a pair's images must have one size (ValueError).  keys: B 64-bit keys, one per pair (aligned=True: both images get
        the pair's key and must have one size, so they get the same coordinates) or 2B, references first (aligned=False); None: keys from
        the pipeline's submission counter.  The samples are a pure function of (seed, key, size, count).  num_repeats=R is the reference's
        validation repeats: every pair is scored R times with the keys sampling.repeat_key(key, r) -- the images cross PCIe once -- and
        the R scores are averaged on the device (validate.average_over_repeats): fp64 (B,) then, else q (B,) as submit() returns it.
        ValueError for a batch over the slot capacity (repeats count against max_pairs and max_patches), before anything is enqueued."""
        refs, dists = _host_images(refs, dists, pairs=True)
        B = len(refs)
        if aligned:
            _aligned_sizes([r.shape[:2] for r in refs], [d.shape[:2] for d in dists])
        kr, kd = pair_keys(keys, self.count, B, aligned)
        counts = patch_counts(patch_count, B)
        weighted = isinstance(sampler, WeightedPatchSampler)
        if weighted and any(r.shape != d.shape for r, d in zip(refs, dists)):
            raise ValueError("WeightedPatchSampler: the two images of a pair must have one size (their difference is taken pixel by pixel)")
        sb = self.plan_sampled([r.shape[:2] for r in refs], [d.shape[:2] for d in dists], counts, counts, kr, kd, num_repeats,
                               scale_num_samples_ratio)
        if weighted:
            out = self._sample_weighted_and_gather(sb, refs + dists, seed, sampler, scale_num_samples_ratio)
        else:
            out = self._sample_and_gather(sb, refs + dists, seed, sampler)
        return mean_over_repeats(self._as_pairs(sb.batch, out), sb.repeats)

    def submit_group_images(self, refs, dists, ref_index, patch_count, keys=None, seed: int = 0, num_repeats: int = 1,
                            sampler: Optional[PatchSampler] = None, scale_num_samples_ratio: float = DEFAULT_NUM_SAMPLES_RATIO,
                            patch_count_dist=None) -> torch.Tensor:
        """submit_group() without coordinates: G references and M distorted images, distorted image m scored against reference
        ref_index[m].  patch_count: one int or G (references); patch_count_dist: one int or M (default: patch_count, which must then be
        one int).  keys: G + M keys, references first (None: from the submission counter); a distorted image with its reference's key and
        size gets its reference's coordinates.  num_repeats as submit_images.  Returns q (M,), fp64 when num_repeats > 1."""
        if isinstance(sampler, WeightedPatchSampler):
            raise NotImplementedError("submit_group_images with WeightedPatchSampler is not built: a group has no pairs of one size to difference")
        refs, dists = _host_images(refs, dists)
        G, M = len(refs), len(dists)
        idx = _ref_indices(ref_index, G, M)
        if patch_count_dist is None:
            if np.ndim(patch_count) != 0:
                raise ValueError("patch_count per reference needs patch_count_dist for the distorted images")
            patch_count_dist = patch_count
        k = as_keys(default_keys(self.count, G + M) if keys is None else keys, G + M)
        sb = self.plan_sampled([r.shape[:2] for r in refs], [d.shape[:2] for d in dists], patch_counts(patch_count, G),
                               patch_counts(patch_count_dist, M), k[:G], k[G:], num_repeats, scale_num_samples_ratio)
        out = self._sample_and_gather(sb, refs + dists, seed, sampler)
        return mean_over_repeats(self._as_group(sb.batch, out, [i + r * G for r in range(sb.repeats) for i in idx]), sb.repeats)
