"""On-device image -> patch tensor: uint8 images + host-sampled coordinates in, the model's
(patches, pos, scales) call tensors out -- the GPU-side half of the reference's loader item
(data/patch_datasets.py:397-409: transform_img x K, get_iqa_patches).  Coordinates stay CPU-sampled (RNG parity is not required)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def _in_range(samples: np.ndarray, levels: Optional[np.ndarray], dims: np.ndarray, num_scales: int, P: int) -> None:
    """THE range rule of a sample, stated once: level in [0, num_scales), 0 <= row <= (H >> level) - P, 0 <= col <= (W >> level) - P.
    samples int [..., 2], levels int [...] or None (all level 0), dims int (H, W) of each sample's image, [..., 2] or [2]; IndexError
    like the reference's numpy fancy-indexing."""
    # numpy on the calling thread: torch CPU operators on these small tensors wake the intra-op thread pool, whose spinning workers
    # then compete with the HIP runtime's own threads -- measured: a pipelined loop fell from 15.4 to 31 ms per batch with the
    # torch form of this check on the host (tools/e2e_probe.py)
    lvl = levels.astype(np.int64) if levels is not None else np.zeros(samples.shape[:-1], dtype=np.int64)
    if ((lvl < 0) | (lvl >= num_scales)).any():
        raise IndexError("scale_ids outside [0, num_scales)")
    lim = (dims >> lvl[..., None]) - P
    if ((samples < 0) | (samples > lim)).any():
        raise IndexError(f"patch sample outside its image's pyramid level (row in [0, h-{P}], col in [0, w-{P}] required)")


def _check_levels(num_scales: int, scale_ids) -> None:
    if not 1 <= num_scales <= 4:
        raise ValueError("1 <= num_scales <= 4")
    if num_scales > 1 and scale_ids is None:
        raise ValueError("scale_ids are required when num_scales > 1")


def _patch_size(patch_size: int) -> int:
    if int(patch_size) not in (16, 8):
        raise ValueError("patch_size must be 16 or 8")
    return int(patch_size)


def check_samples_host(samples: torch.Tensor, scale_ids: Optional[torch.Tensor], H: int, W: int, num_scales: int = 1, patch_size: int = 16) -> None:
    """The range check of the sampled coordinates (IndexError like the reference's numpy fancy-indexing).  Host tensors are checked where
    they are and cost no GPU synchronisation (a pipelined loader calls this BEFORE the copy and passes validate=False below); device
    tensors are read back, which synchronises."""
    to_np = lambda a: a.detach().numpy() if a.device.type == "cpu" else a.detach().cpu().numpy()
    _in_range(to_np(samples), to_np(scale_ids) if scale_ids is not None else None, np.array([H, W], dtype=np.int64), num_scales,
              int(patch_size))


def extract_patches(images_u8: torch.Tensor, samples: torch.Tensor, scale_ids: Optional[torch.Tensor] = None, num_scales: int = 1,
                    flips: Optional[torch.Tensor] = None, mean: Sequence[float] = (0.5, 0.5, 0.5), std: Sequence[float] = (0.5, 0.5, 0.5),
                    patch_size: int = 16, validate: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """images_u8 [NI, H, W, 3] uint8 (cuda); samples [NI, N, 2] int32 (row, col at the patch's own scale);
    scale_ids [NI, N] int32 (required when num_scales > 1, patches of scale s index pyramid level s); flips [NI, 2] int32
    (hflip, vflip) or None; patch_size P = 16 (ViT-B16 / ViT-L16) or 8 (ViT-B8).  Returns patches [NI, N, 3, P, P] f32, pos [NI, N, 2] f32,
    scales [NI, N] f32 or None.  validate=False skips the device-side range check of the samples (one reduction + a stream
    synchronisation): for a pipelined loader that has checked them on the host before the copy (check_samples_host)."""
    lib = _lib.load()
    dev = images_u8.device
    if dev.type != "cuda":
        raise RuntimeError("extract_patches runs on the GPU only (no CPU fallback on the product path)")
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError("images_u8 must be uint8 [NI, H, W, 3]")
    NI, H, W, _ = images_u8.shape
    N = samples.shape[1]
    if tuple(samples.shape) != (NI, N, 2):
        raise ValueError("samples must be int32 [NI, N, 2]")
    _check_levels(num_scales, scale_ids)
    P = _patch_size(patch_size)
    # Range checks the reference gets for free from numpy fancy-indexing (an out-of-range patch raises IndexError there); the
    # gather kernel itself does not bounds-check.  One small reduction + sync per call, on the loader side of the pipeline.
    if (H >> (num_scales - 1)) < P or (W >> (num_scales - 1)) < P:
        raise ValueError(f"pyramid level {num_scales - 1} of a {H}x{W} image is smaller than one {P}x{P} patch")
    if scale_ids is not None and tuple(scale_ids.shape) != (NI, N):
        raise ValueError("scale_ids must be int32 [NI, N]")
    if validate:
        check_samples_host(samples, scale_ids, H, W, num_scales, P)
    images_u8 = images_u8.contiguous()
    samples = samples.to(device=dev, dtype=torch.int32).contiguous()
    sid = scale_ids.to(device=dev, dtype=torch.int32).contiguous() if scale_ids is not None else None
    fl = flips.to(device=dev, dtype=torch.int32).contiguous() if flips is not None else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        levels = [torch.empty(NI, 3, H, W, device=dev, dtype=torch.float32)]
        m = (C.c_float * 3)(*mean)
        s = (C.c_float * 3)(*std)
        _lib.check(lib.vtq_k_image_normalize(images_u8.data_ptr(), levels[0].data_ptr(), NI, H, W, fl.data_ptr() if fl is not None else None,
                                             m, s, stream))
        for _ in range(1, num_scales):
            h, w = levels[-1].shape[2:]
            nxt = torch.empty(NI, 3, h // 2, w // 2, device=dev, dtype=torch.float32)
            _lib.check(lib.vtq_k_avgpool2(levels[-1].data_ptr(), nxt.data_ptr(), NI * 3, h, w, stream))
            levels.append(nxt)
        patches = torch.empty(NI, N, 3, P, P, device=dev, dtype=torch.float32)
        pos = torch.empty(NI, N, 2, device=dev, dtype=torch.float32)
        scales = torch.empty(NI, N, device=dev, dtype=torch.float32) if num_scales > 1 else None
        ptrs = (C.c_void_p * len(levels))(*[l.data_ptr() for l in levels])
        hs = (C.c_int32 * len(levels))(*[l.shape[2] for l in levels])
        ws = (C.c_int32 * len(levels))(*[l.shape[3] for l in levels])
        _lib.check(lib.vtq_k_gather_patches(ptrs, hs, ws, len(levels), samples.data_ptr(), sid.data_ptr() if sid is not None else None,
                                            patches.data_ptr(), pos.data_ptr(), scales.data_ptr() if scales is not None else None, NI, N,
                                            P, stream))
    return patches, pos, scales


# ---- images of different sizes (include/vtamiq_hip_images.h, csrc/patches_ragged.hip) -------------------------------------------------------
class ImageTables(NamedTuple):
    """Host tables of one batch of NI images of different sizes (image_tables)."""
    img_off: np.ndarray       # int64 [NI]      byte offset of image i in the flat buffer (images packed back to back, in order)
    H: np.ndarray             # int32 [NI]
    W: np.ndarray             # int32 [NI]
    row0: np.ndarray          # int32 [NI + 1]  patch-row prefix: image i owns rows [row0[i], row0[i + 1])
    tab: np.ndarray           # int32 [NI, 4]   (img_off low word, high word, H, W): what the kernel reads
    patch_img: np.ndarray     # int32 [total]   the image of every patch row
    image_bytes: int          # sum of 3 H W times the element size (1 for uint8 images)
    total: int                # row0[NI]


def _sizes(sizes) -> np.ndarray:
    sz = np.asarray([(int(h), int(w)) for h, w in sizes], dtype=np.int64).reshape(-1, 2)
    if sz.shape[0] < 1 or (sz < 1).any():
        raise ValueError("sizes: at least one (H, W), both >= 1")
    return sz


def image_tables(sizes, lengths, elem: int = 1) -> ImageTables:
    """The offset, prefix and image-index tables of NI images [(H_i, W_i) ...] with lengths[i] >= 0 patches each, on the host (numpy only).
    elem: bytes per pixel element -- 1 for uint8 images, 4 or 2 for the float planes of extract_patches_planar; the offsets are bytes."""
    sz = _sizes(sizes)
    ln = np.asarray(lengths)
    if ln.shape != (sz.shape[0],) or ln.dtype.kind not in "iu":
        raise ValueError("lengths: one integer per image")
    ln = ln.astype(np.int64)
    if (ln < 0).any():
        raise ValueError("lengths: >= 0")
    nbytes = 3 * sz[:, 0] * sz[:, 1] * int(elem)
    off = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    row0 = np.concatenate([[0], np.cumsum(ln)])
    if row0[-1] > 0x7fffffff or (sz > 0x7fffffff).any():
        raise ValueError("more than 2^31 - 1 patches or pixels per side")
    tab = np.empty((sz.shape[0], 4), np.int32)
    tab[:, :2] = off.astype("<i8").view("<i4").reshape(-1, 2)
    tab[:, 2:] = sz
    return ImageTables(off, sz[:, 0].astype(np.int32), sz[:, 1].astype(np.int32), row0.astype(np.int32), tab,
                       np.repeat(np.arange(sz.shape[0], dtype=np.int32), ln), int(nbytes.sum()), int(row0[-1]))


def table_rows(t: ImageTables, rows, lengths) -> ImageTables:
    """Tables whose row k is image rows[k] of `t` with lengths[k] patches: an image listed more than once (validation repeats) keeps ONE
    copy of its pixels, every listing its own patch rows."""
    rows, lengths = np.asarray(rows, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    row0 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return ImageTables(t.img_off[rows], t.H[rows], t.W[rows], row0, np.ascontiguousarray(t.tab[rows]),
                       np.repeat(np.arange(len(rows), dtype=np.int32), lengths), t.image_bytes, int(row0[-1]))


def check_samples_host_varlen(samples, scale_ids, sizes, lengths, num_scales: int = 1, patch_size: int = 16) -> None:
    """check_samples_host for images of different sizes: samples (total, 2) and scale_ids (total,) or None are the per-image lists
    concatenated, image i = (H_i, W_i) owning lengths[i] rows.  Every sample must lie inside ITS image's level -- a small image may use fewer levels than
    num_scales; a sample on a level of its image that is smaller than one patch has no valid position -- IndexError otherwise, like the
    reference's fancy indexing.  numpy on the calling thread (_in_range says why)."""
    _check_levels(num_scales, scale_ids)
    sz = _sizes(sizes)
    ln = np.asarray(lengths, dtype=np.int64)
    smp = np.asarray(samples)
    if ln.shape != (sz.shape[0],) or smp.shape != (int(ln.sum()), 2):
        raise ValueError("samples must be (sum(lengths), 2), lengths one count per image")
    lvl = np.asarray(scale_ids) if scale_ids is not None else None
    if lvl is not None and lvl.shape != (smp.shape[0],):
        raise ValueError("scale_ids must be (sum(lengths),)")
    _in_range(smp, lvl, np.repeat(sz, ln, axis=0), num_scales, int(patch_size))           # dims (total, 2): the image of every row


def _gather(flat: torch.Tensor, tables: ImageTables, dev_tab, dev_patch_img, samples, scale_ids, flips, num_scales: int, mean, std,
            patch_size: int):
    """The launch of either gather on the current stream, chosen by the dtype of `flat`: vtq_k_gather_patches_u8 for uint8 HWC bytes,
    vtq_k_gather_patches_planar for float CHW planes.  The two entries take the same arguments but for the pixel dtype."""
    lib = _lib.load()
    dev = flat.device
    P, T = int(patch_size), tables.total
    with torch.cuda.device(dev):
        patches = torch.empty(T, 3, P, P, device=dev, dtype=torch.float32)
        pos = torch.empty(T, 2, device=dev, dtype=torch.float32)
        scales = torch.empty(T, device=dev, dtype=torch.float32) if num_scales > 1 else None
        as_p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        image = (flat.data_ptr(), flat.numel() * flat.element_size())
        rest = (dev_tab.data_ptr(), dev_patch_img.data_ptr(), as_p(tables.img_off, C.c_int64),
                as_p(tables.H, C.c_int32), as_p(tables.W, C.c_int32), as_p(tables.row0, C.c_int32), len(tables.H), samples.data_ptr(),
                scale_ids.data_ptr() if scale_ids is not None else None, flips.data_ptr() if flips is not None else None,
                (C.c_float * 3)(*mean), (C.c_float * 3)(*std), patches.data_ptr(), pos.data_ptr(),
                scales.data_ptr() if scales is not None else None, P, num_scales, torch.cuda.current_stream(dev).cuda_stream)
        if flat.dtype == torch.uint8:
            _lib.check(lib.vtq_k_gather_patches_u8(*image, *rest))
        else:
            _lib.check(lib.vtq_k_gather_patches_planar(*image, _lib.PIXEL_DTYPES[str(flat.dtype).split(".")[-1]], *rest))
    return patches, pos, scales


def gather_patches_u8(flat: torch.Tensor, tables: ImageTables, dev_tab: torch.Tensor, dev_patch_img: torch.Tensor, samples: torch.Tensor,
                      scale_ids: Optional[torch.Tensor], flips: Optional[torch.Tensor], num_scales: int, mean, std, patch_size: int):
    """The launch itself (vtq_k_gather_patches_u8) on the current stream: every tensor is on the device already, `tables` are the host
    arrays dev_tab / dev_patch_img were copied from.  Nothing here copies or synchronises."""
    if flat.dtype != torch.uint8:
        raise ValueError("gather_patches_u8 takes uint8 bytes")
    return _gather(flat, tables, dev_tab, dev_patch_img, samples, scale_ids, flips, num_scales, mean, std, patch_size)


PLANAR_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def gather_patches_planar(flat: torch.Tensor, tables: ImageTables, dev_tab: torch.Tensor, dev_patch_img: torch.Tensor, samples: torch.Tensor,
                          scale_ids: Optional[torch.Tensor], flips: Optional[torch.Tensor], num_scales: int, mean, std, patch_size: int):
    """gather_patches_u8 for float CHW planes (vtq_k_gather_patches_planar): flat is 1-D float32 / float16 / bfloat16 and `tables` were made
    with elem=flat.element_size().  Nothing here copies or synchronises."""
    if flat.dtype not in PLANAR_DTYPES:
        raise ValueError("gather_patches_planar takes float32, float16 or bfloat16 planes")
    return _gather(flat, tables, dev_tab, dev_patch_img, samples, scale_ids, flips, num_scales, mean, std, patch_size)


def _extract_flat(flat: torch.Tensor, sizes, samples, lengths, scale_ids, num_scales, flips, mean, std, patch_size, validate):
    """The part extract_patches_varlen and extract_patches_planar share: `flat` holds the images back to back (uint8 HWC or float CHW),
    sizes their (H_i, W_i).  Table building, shape and range checks, the upload of host arguments and the launch."""
    dev = flat.device
    P = _patch_size(patch_size)
    _check_levels(num_scales, scale_ids)
    lengths = [int(n) for n in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
    tables = image_tables(sizes, lengths, flat.element_size())
    if tables.total < 1:
        raise ValueError("no patches: sum(lengths) must be at least 1")
    if flat.numel() * flat.element_size() != tables.image_bytes:
        raise ValueError(f"the flat image tensor has {flat.numel() * flat.element_size()} bytes, the sizes need {tables.image_bytes}")
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if tuple(samples.shape) != (tables.total, 2):
        raise ValueError("samples must be int32 (sum(lengths), 2)")
    if scale_ids is not None and tuple(scale_ids.shape) != (tables.total,):
        raise ValueError("scale_ids must be int32 (sum(lengths),)")
    if flips is not None and tuple(flips.shape) != (len(lengths), 2):
        raise ValueError("flips must be int32 (NI, 2)")
    if validate:
        check_samples_host_varlen(to_np(samples), to_np(scale_ids) if scale_ids is not None else None, sizes, lengths, num_scales, P)
    on_dev = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.int32).contiguous()
    return _gather(flat, tables, on_dev(tables.tab), on_dev(tables.patch_img), on_dev(samples),
                   on_dev(scale_ids) if scale_ids is not None else None, on_dev(flips) if flips is not None else None,
                   num_scales, mean, std, P)


def extract_patches_varlen(images, samples, lengths, scale_ids=None, num_scales: int = 1, flips=None,
                           mean: Sequence[float] = (0.5, 0.5, 0.5), std: Sequence[float] = (0.5, 0.5, 0.5), patch_size: int = 16,
                           validate: bool = True, sizes=None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """extract_patches for NI images of DIFFERENT sizes in one launch, without a normalised copy or a pyramid of any image.
      images     a list of uint8 [H_i, W_i, 3] cuda tensors (concatenated here, on the device), or ONE flat uint8 cuda tensor holding them
                 back to back, with sizes=[(H_i, W_i) ...]
      samples    int32 (sum(lengths), 2): the images' sample lists concatenated, (row, col) at each patch's own level; lengths: NI counts
      scale_ids  int32 (sum(lengths),), required when num_scales > 1;  flips int32 (NI, 2) = (hflip, vflip) or None
    Returns patches (sum, 3, P, P), pos (sum, 2), scales (sum,) or None -- fp32, concatenated per image: what forward_varlen and
    forward_group(..., lengths=) take.  Every element has the bits extract_patches gives for that image alone.  validate=True range-checks
    the samples on the host (check_samples_host_varlen; samples on the device are read back, which synchronises); a pipelined loader checks
    its host copy before the upload and passes validate=False (pipeline.ImagePairVarlenPipeline)."""
    if isinstance(images, torch.Tensor):
        if sizes is None:
            raise ValueError("a flat image tensor needs sizes=[(H, W) ...]")
        flat = images
    else:
        if sizes is not None:
            raise ValueError("sizes= goes with a flat image tensor; a list of images carries its own")
        images = list(images)
        if not images or any(not isinstance(i, torch.Tensor) or i.dim() != 3 or i.shape[-1] != 3 for i in images):
            raise ValueError("images must be a non-empty list of uint8 [H, W, 3] tensors")
        sizes = [tuple(i.shape[:2]) for i in images]
        flat = images[0]
    dev = flat.device
    if dev.type != "cuda":
        raise RuntimeError("extract_patches_varlen runs on the GPU only (no CPU fallback on the product path)")
    if not isinstance(images, torch.Tensor):
        if any(i.dtype != torch.uint8 or i.device != dev for i in images):
            raise ValueError("images must be uint8 tensors on one device")
        flat = torch.cat([i.contiguous().reshape(-1) for i in images])
    if flat.dtype != torch.uint8 or flat.dim() != 1:
        raise ValueError("the flat image tensor must be uint8 and one-dimensional")
    return _extract_flat(flat, sizes, samples, lengths, scale_ids, num_scales, flips, mean, std, patch_size, validate)


# ---- float images resident on the device (include/vtamiq_hip_tensors.h, csrc/patches_planar.hip) ------------------------------------------
class ResidentImages(NamedTuple):
    """Images that are on the device, inspected on the host without enqueuing anything (resident_images)."""
    sizes: list               # NI (H, W)
    dtype: torch.dtype        # uint8: HWC bytes (the u8 gather); float32 / float16 / bfloat16: CHW planes (the planar gather)
    device: torch.device
    parts: list               # the tensors as given: one batch or flat tensor, or the list's images

    def flat(self) -> torch.Tensor:
        """The images back to back in ONE 1-D tensor: a view of a batch or flat tensor (no copy), the concatenation of a list (one copy of
        the images, on the device and the current stream)."""
        if len(self.parts) == 1 and self.parts[0].is_contiguous():
            return self.parts[0].view(-1)
        return torch.cat([i.contiguous().reshape(-1) for i in self.parts])


def resident_images(images, sizes=None, what: str = "images", u8: bool = False) -> ResidentImages:
    """The input forms of extract_patches_planar (and, with u8=True, their uint8 HWC counterparts), checked on the host:
      one contiguous batch tensor (NI, 3, H, W) of float pixels -- or (NI, H, W, 3) of uint8 --, used in place;
      a list of (3, H_i, W_i) float tensors -- or (H_i, W_i, 3) uint8 ones -- of one dtype on one device, concatenated by flat();
      one flat 1-D tensor with sizes=[(H_i, W_i) ...], used in place.
    Refused: CPU tensors (RuntimeError); float64 and integer pixels other than uint8 (TypeError); a batch tensor that is not contiguous in
    its own order -- strided or channels_last -- naming .contiguous(): nothing here copies a strided batch silently (ValueError, like every
    other malformed argument)."""
    if isinstance(images, torch.Tensor):
        ts = [images]
    else:
        ts = list(images)
        if not ts or any(not isinstance(i, torch.Tensor) for i in ts):
            raise ValueError(f"{what}: a tensor or a non-empty list of tensors")
    dev, dtype = ts[0].device, ts[0].dtype
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: a {dev.type} tensor; images that are resident on the GPU are taken (no CPU fallback on the product path)")
    if dtype not in PLANAR_DTYPES and not (u8 and dtype == torch.uint8):
        raise TypeError(f"{what}: float32, float16 or bfloat16 pixels{' or uint8 bytes' if u8 else ''}, not {dtype}")
    if any(i.device != dev or i.dtype != dtype for i in ts):
        raise ValueError(f"{what}: tensors of one dtype on one device")
    hwc = dtype == torch.uint8
    form = "(H, W, 3)" if hwc else "(3, H, W)"
    hw = (lambda t: tuple(int(d) for d in t.shape[-3:-1])) if hwc else (lambda t: tuple(int(d) for d in t.shape[-2:]))
    chan = (lambda t: t.shape[-1]) if hwc else (lambda t: t.shape[-3])
    if not isinstance(images, torch.Tensor):
        if sizes is not None:
            raise ValueError("sizes= goes with a flat image tensor; a list of images carries its own")
        if any(i.dim() != 3 or chan(i) != 3 for i in ts):
            raise ValueError(f"{what}: a list of {form} tensors")
        return ResidentImages([hw(i) for i in ts], dtype, dev, ts)
    if images.dim() == 1:
        if sizes is None:
            raise ValueError("a flat image tensor needs sizes=[(H, W) ...]")
        if not images.is_contiguous():
            raise ValueError(f"{what}: the flat tensor is strided: pass images.contiguous()")
        return ResidentImages([(int(h), int(w)) for h, w in sizes], dtype, dev, ts)
    if sizes is not None:
        raise ValueError("sizes= goes with a flat image tensor; a batch tensor carries its own")
    if images.dim() != 4 or chan(images) != 3 or images.shape[0] < 1:
        raise ValueError(f"{what}: a batch tensor must be (NI, {form[1:-1]}), NI >= 1")
    if not images.is_contiguous():
        raise ValueError(f"{what}: the batch tensor is not contiguous in (NI, {form[1:-1]}) order (strided or channels_last): "
                         "pass images.contiguous()")
    return ResidentImages([hw(images)] * images.shape[0], dtype, dev, ts)


def extract_patches_planar(images, samples, lengths, scale_ids=None, num_scales: int = 1, flips=None,
                           mean: Sequence[float] = (0.5, 0.5, 0.5), std: Sequence[float] = (0.5, 0.5, 0.5), patch_size: int = 16,
                           validate: bool = True, sizes=None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """extract_patches_varlen for FLOAT images that are already on the device, e.g. the output of another model: float32 / float16 /
    bfloat16 pixels in CHW order, gathered as they are -- no quantisation to 8 bits, no permute, no host copy.
      images     ONE contiguous cuda tensor (NI, 3, H, W), used in place with no copy;  or a list of (3, H_i, W_i) cuda tensors of one dtype,
                 which are CONCATENATED here on the device (one copy of the images: keep them in one flat tensor to avoid it);  or ONE flat
                 1-D tensor holding the images' planes back to back, with sizes=[(H_i, W_i) ...], used in place
      the other arguments, the returns and the checks are those of extract_patches_varlen
    Level 0 is ((float)x - mean[c]) / std[c], the pooled levels the nested 2 x 2 means of it: the bits oracle.patch_oracle gives for the
    normalised image.  A pixel scale of [0, 1] is the caller's (the reference's to_tensor leaves float arrays unscaled too)."""
    res = resident_images(images, sizes)
    return _extract_flat(res.flat(), res.sizes, samples, lengths, scale_ids, num_scales, flips, mean, std, patch_size, validate)
