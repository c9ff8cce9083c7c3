"""Host side of scoring image tensors that are already on the device: the planar gather's entry (include/vtamiq_hip_tensors.h),
vtamiq_amd.patches.extract_patches_planar / resident_images and vtamiq_amd.ImageMetric.  No GPU: the entry's refusals are decided on host
arrays, the Python refusals on shapes, dtypes and devices -- before the library is looked at."""
import ctypes
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

from vtamiq_amd import ImageMetric, _lib, patches
from vtamiq_amd.patches import extract_patches_planar, image_tables, resident_images, table_rows
from vtamiq_amd.sampling import WeightedPatchSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vtq_k_gather_patches_planar"


def test_tensors_header_declares_exactly_the_bound_entry_and_the_library_exports_it():
    from vtamiq_amd import build
    header = open(os.path.join(ROOT, "include", "vtamiq_hip_tensors.h")).read()
    declared = set(re.findall(r"\b(vtq_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.TENSOR_SIGNATURES) == {ENTRY}
    for other in ("vtamiq_hip.h", "vtamiq_hip_images.h"):
        assert ENTRY not in open(os.path.join(ROOT, "include", other)).read(), other
    rest = (_lib.SIGNATURES, _lib.ROLLOUT_SIGNATURES, _lib.IMAGE_SIGNATURES, _lib.SAMPLER_SIGNATURES, _lib.WEIGHTED_SAMPLER_SIGNATURES, _lib.FP8_SIGNATURES)
    assert not any(ENTRY in s for s in rest)
    assert "patches_planar.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, ENTRY)
    lib.vtq_abi_version.restype = ctypes.c_int
    assert lib.vtq_abi_version() == _lib.ABI_VERSION == 10
    nargs = len(re.search(ENTRY + r"\((.*?)\);", header, re.S).group(1).split(","))
    assert nargs == len(_lib.TENSOR_SIGNATURES[ENTRY][1]) == len(_lib.IMAGE_SIGNATURES["vtq_k_gather_patches_u8"][1]) + 1
    codes = dict(re.findall(r"#define VTQ_PIXEL_(\w+) (\d)", header))
    assert {k: int(v) for k, v in codes.items()} == {"F32": 0, "F16": 1, "BF16": 2}
    assert _lib.PIXEL_DTYPES == {"float32": 0, "float16": 1, "bfloat16": 2}


def test_tables_in_element_sizes_and_repeated_rows():
    sizes, lengths = [(16, 16), (17, 33), (37, 53)], [1, 2, 5]
    one = image_tables(sizes, lengths)
    for elem in (2, 4):
        t = image_tables(sizes, lengths, elem)
        assert (t.img_off == one.img_off * elem).all() and t.image_bytes == one.image_bytes * elem
        assert (t.row0 == one.row0).all() and (t.patch_img == one.patch_img).all() and (t.tab[:, 2:] == one.tab[:, 2:]).all()
        assert all((int(t.tab[i, 0]) & 0xffffffff) | (int(t.tab[i, 1]) << 32) == t.img_off[i] for i in range(3))
    half = image_tables(sizes, lengths, 2)
    assert half.img_off[2] % 4 == 2, "17 x 33 x 3 fp16 elements are 3366 bytes: the image behind starts 2-byte aligned only"
    rows = [0, 1, 2, 0, 1, 2]
    rep = table_rows(half, rows, [1, 2, 5, 1, 2, 5])
    assert (rep.img_off == half.img_off[rows]).all() and rep.total == 16 and rep.image_bytes == half.image_bytes
    assert rep.row0.tolist() == [0, 1, 3, 8, 9, 11, 16] and rep.patch_img.tolist() == [0, 1, 1] + [2] * 5 + [3, 4, 4] + [5] * 5


def test_entry_refuses_bad_arguments_without_a_device():
    """Every refusal of include/vtamiq_hip_tensors.h is decided on HOST arrays before any HIP call: provoked here with made-up device
    addresses that are never dereferenced.  Every message begins with the entry's name."""
    lib = _lib.load()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ptr = lambda a, ty: a.ctypes.data_as(ctypes.POINTER(ty))
    DEV = 0x10000                                                    # stands for a device address: non-NULL, 16-byte aligned

    def call(elem, **kw):
        t = image_tables([(16, 16), (17, 33)], [1, 2], elem)
        a = dict(images=DEV, image_bytes=t.image_bytes, dtype={4: 0, 2: 1}[elem], tab=DEV, patch_img=DEV, img_off=t.img_off, H=t.H, W=t.W,
                 row0=t.row0, NI=2, samples=DEV, scale_ids=None, flips=None, mean=f3, std=f3, patches=DEV, pos=DEV, scales=None, P=16, ns=1)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        host = lambda k, ty: ptr(a[k], ty) if a[k] is not None else None
        rc = getattr(lib, ENTRY)(a["images"], a["image_bytes"], a["dtype"], a["tab"], a["patch_img"], host("img_off", ctypes.c_int64),
                                 host("H", ctypes.c_int32), host("W", ctypes.c_int32), host("row0", ctypes.c_int32), a["NI"], a["samples"],
                                 a["scale_ids"], a["flips"], a["mean"], a["std"], a["patches"], a["pos"], a["scales"], a["P"], a["ns"], None)
        return rc, lib.vtq_last_error().decode()

    i32, i64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64))
    cases = {k: {k: None} for k in ("images", "tab", "patch_img", "img_off", "H", "W", "row0", "samples", "mean", "std", "patches", "pos")}
    cases.update({                                                   # everything the u8 entry refuses ...
        "NI < 1": dict(NI=0), "row0 decreases": dict(row0=i32(0, 2, 1)), "row0[0] != 0": dict(row0=i32(1, 2, 3)),
        "no patches": dict(row0=i32(0, 0, 0)), "P": dict(P=12), "num_scales 0": dict(ns=0), "num_scales 5": dict(ns=5, scale_ids=DEV),
        "scale_ids NULL": dict(ns=2), "image smaller than P": dict(H=i32(15, 17)), "P = 16 on an 8-row image": dict(H=i32(8, 17)),
        "image leaves the buffer by one byte": dict(image_bytes=lambda t: t.image_bytes - 1),
        "image leaves the buffer by one element": dict(W=i32(16, 34)),
        "negative offset": dict(img_off=lambda t: i64(-t.img_off[1], t.img_off[1])), "tab unaligned": dict(tab=DEV + 4),
        "negative buffer": dict(image_bytes=-1),
        # ... and what the pixel format adds
        "dtype 3": dict(dtype=3), "dtype -1": dict(dtype=-1), "dtype 7 (a torch code)": dict(dtype=7)})
    for elem in (4, 2):
        for name, kw in cases.items():
            rc, msg = call(elem, **kw)
            assert rc != 0 and msg.startswith(ENTRY + ":"), (elem, name, rc, msg)
        for off in range(1, elem):                                   # an offset that is not a multiple of the element size
            rc, msg = call(elem, img_off=lambda t: i64(0, t.img_off[1] + off), image_bytes=lambda t: t.image_bytes + elem)
            assert rc != 0 and msg.startswith(ENTRY + ":") and "multiple" in msg, (elem, off, msg)
    rc, msg = call(2, dtype=0)                                       # fp16-sized offsets and buffer read as fp32
    assert rc != 0 and msg.startswith(ENTRY + ":")


# ---- the Python refusals: before any library call -------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """A host tensor that says it lives on the GPU: what the shape / dtype / layout checks see of a resident image, on a machine without one.
    A call that got past its refusals would reach the library, which the tests below replace by a trap."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnGpu)


@pytest.fixture
def no_library(monkeypatch):
    def trap(*a, **k):
        raise AssertionError("the library was called before the refusal")
    monkeypatch.setattr(_lib, "load", trap)


def _metric(**kw):
    model = types.SimpleNamespace(spec=types.SimpleNamespace(patch_size=16))
    return ImageMetric(model, patch_count=20, **kw)


def test_resident_images_reads_sizes_from_the_shapes():
    r = resident_images(gpu(4, 3, 37, 53, dtype=torch.float16))
    assert r.sizes == [(37, 53)] * 4 and r.dtype == torch.float16 and r.device.type == "cuda"
    r = resident_images([gpu(3, 16, 16), gpu(3, 17, 33)])
    assert r.sizes == [(16, 16), (17, 33)]
    r = resident_images(gpu(3 * 16 * 16 + 3 * 17 * 33), sizes=[(16, 16), (17, 33)])
    assert r.sizes == [(16, 16), (17, 33)]
    r = resident_images(gpu(2, 48, 64, 3, dtype=torch.uint8), u8=True)
    assert r.sizes == [(48, 64)] * 2 and r.dtype == torch.uint8
    assert resident_images([gpu(48, 64, 3, dtype=torch.uint8), gpu(17, 33, 3, dtype=torch.uint8)], u8=True).sizes == [(48, 64), (17, 33)]


def test_python_refusals_come_before_any_library_call(no_library):
    ok = gpu(2, 3, 32, 32)
    smp, lens = torch.zeros(2, 2, dtype=torch.int32), [1, 1]
    cl = torch.zeros(2, 3, 32, 32).to(memory_format=torch.channels_last).as_subclass(OnGpu)
    strided = torch.zeros(2, 3, 32, 64)[..., ::2].as_subclass(OnGpu)
    assert not cl.is_contiguous() and not strided.is_contiguous()
    m = _metric()
    for call in (lambda x: extract_patches_planar(x, smp, lens), lambda x: m(x, ok), lambda x: m(ok, x),
                 lambda x: m.group(x, ok, [0, 0]), lambda x: m.group(ok, x, [0, 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.zeros(2, 3, 32, 32))                          # a CPU tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call([torch.zeros(3, 32, 32)] * 2)
        for dtype in (torch.float64, torch.int32, torch.int8, torch.int16, torch.int64, torch.bool):
            with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
                call(gpu(2, 3, 32, 32, dtype=dtype))
        for bad in (cl, strided):
            with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
                call(bad)
        with pytest.raises(ValueError):
            call(gpu(2, 4, 32, 32))                                  # four channels
        with pytest.raises(ValueError):
            call([gpu(3, 32, 32), gpu(3, 32, 32, dtype=torch.float16)])
        with pytest.raises(ValueError):
            call([])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        extract_patches_planar(gpu(2, 32, 32, 3, dtype=torch.uint8), smp, lens)          # uint8 belongs to extract_patches_varlen
    with pytest.raises(ValueError, match="sizes"):
        extract_patches_planar(gpu(3 * 32 * 32), smp[:1], [1])
    with pytest.raises(ValueError, match="sizes"):
        extract_patches_planar(ok, smp, lens, sizes=[(32, 32)] * 2)
    with pytest.raises(ValueError, match="bytes"):
        extract_patches_planar(gpu(3 * 32 * 32 + 1), smp[:1], [1], sizes=[(32, 32)])
    assert m.count == 0


def test_metric_refusals_come_before_any_library_call(no_library):
    ok, half = gpu(2, 3, 32, 32), gpu(2, 3, 32, 32, dtype=torch.float16)
    u8 = gpu(2, 32, 32, 3, dtype=torch.uint8)
    m = _metric()
    with pytest.raises(TypeError, match="one dtype"):
        m(ok, half)
    with pytest.raises(TypeError, match="one dtype"):
        m(u8, ok)
    with pytest.raises(TypeError, match="one dtype"):
        m.group(half, ok, [0, 1])
    with pytest.raises(ValueError, match="aligned sampling"):
        m([gpu(3, 32, 32), gpu(3, 48, 64)], [gpu(3, 32, 32), gpu(3, 64, 48)])
    with pytest.raises(ValueError, match="aligned sampling"):
        m(gpu(2, 32, 48, 3, dtype=torch.uint8), gpu(2, 48, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="smaller than one"):
        m(gpu(2, 3, 15, 32), gpu(2, 3, 15, 32))
    with pytest.raises(ValueError, match="smaller than one"):
        m([gpu(3, 32, 32), gpu(3, 32, 15)], [gpu(3, 32, 32), gpu(3, 32, 15)], aligned=False)
    with pytest.raises(ValueError, match="smaller than one"):
        m.group([gpu(3, 32, 32)], [gpu(3, 8, 32)], [0])
    with pytest.raises(ValueError):
        m(ok, gpu(3, 3, 32, 32))                                     # two references, three distorted images
    with pytest.raises(ValueError, match="keys"):
        m(ok, ok, keys=[1, 2, 3])
    with pytest.raises(ValueError, match="keys"):
        m(ok, ok, keys=[1, 2], aligned=False)
    with pytest.raises(ValueError, match="ref_index"):
        m.group(ok, ok, [0, 2])
    with pytest.raises(ValueError, match="patch_count"):
        ImageMetric(m.model, patch_count=2, num_scales=3)(ok, ok)    # fewer patches than scales
    with pytest.raises(ValueError):
        ImageMetric(m.model, patch_count=[20, 20, 20])(ok, ok)       # three counts for two pairs
    with pytest.raises(ValueError, match="patch_count_dist"):
        ImageMetric(m.model, patch_count=[20, 20]).group(ok, ok, [0, 1])
    with pytest.raises(ValueError):
        ImageMetric(m.model, num_repeats=0)
    with pytest.raises(ValueError):
        ImageMetric(m.model, num_scales=5, patch_count=20)(ok, ok)
    for images in ((ok, ok), (half, half)):
        with pytest.raises(NotImplementedError, match="defined on bytes"):
            _metric(sampler=WeightedPatchSampler(diff_weight=1.0))(*images)
    for images in ((ok, ok), (half, half)):
        with pytest.raises(NotImplementedError, match="defined on bytes"):
            _metric(sampler=WeightedPatchSampler(diff_weight=1.0)).group(*images, [0, 1])
    with pytest.raises(ValueError, match="one size"):                # uint8: sampled where the pair differs, pixel by pixel
        _metric(sampler=WeightedPatchSampler(diff_weight=1.0))([gpu(32, 48, 3, dtype=torch.uint8)], [gpu(48, 32, 3, dtype=torch.uint8)],
                                                               keys=[1, 2], aligned=False)
    with pytest.raises(ValueError, match="smaller than one"):
        _metric(sampler=WeightedPatchSampler(diff_weight=1.0))(gpu(2, 15, 32, 3, dtype=torch.uint8), gpu(2, 15, 32, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="WeightedPatchSampler"):
        _metric(sampler=WeightedPatchSampler(diff_weight=1.0)).group(u8, u8, [0, 1])
    assert m.count == 0


def test_an_input_that_requires_grad_is_warned_about(no_library):
    """The warning comes with the other host checks; the call then goes on towards the device, which this machine need not have."""
    x = torch.zeros(2, 3, 32, 32, requires_grad=True).as_subclass(OnGpu)
    assert x.requires_grad
    with pytest.warns(UserWarning, match="without an autograd graph"):
        with pytest.raises(Exception):
            _metric()(gpu(2, 3, 32, 32), x)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad(), pytest.raises(Exception):
            _metric()(gpu(2, 3, 32, 32), x)
    assert patches.PLANAR_DTYPES == (torch.float32, torch.float16, torch.bfloat16)
