"""Scoring image tensors that are already on the device: vtq_k_gather_patches_planar (include/vtamiq_hip_tensors.h),
vtamiq_amd.patches.extract_patches_planar and vtamiq_amd.ImageMetric, on the GPU.

The contracts every test turns on: a float image's patches have the BITS of the CPU oracle (oracle/patch_oracle.py) on that image's
normalised pixels alone -- whatever its dtype, whatever else is in the batch, wherever it starts in the buffer --, and ImageMetric's scores
the bits of forward_varlen / forward_group(lengths=) on patches gathered at the coordinates the sampler's numpy restatement
(tests/sampler_model.py) gives.  The shapes are the catalogue of tests/image_varlen_cases.py."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from oracle import patch_oracle as PO
from tests import image_varlen_cases as IC
from tests import sampler_model as SM
from tests.footprint import Arena, arena_bytes
from tests.test_gpu_streams import Busy
from vtamiq_amd import VTAMIQ, ImageMetric, _lib, synth
from vtamiq_amd.patches import extract_patches_planar, extract_patches_varlen, image_tables
from vtamiq_amd.pipeline import ImagePairVarlenPipeline
from vtamiq_amd.sampling import repeat_key
from vtamiq_amd.validate import average_over_repeats

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16, I32, U8 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.uint8
DTYPES = {"fp32": F32, "fp16": F16, "bf16": BF16}
CODE = {F32: 0, F16: 1, BF16: 2}
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
NS = IC.NUM_SCALES


def make_planar(sizes, seed, dtype):
    """CHW images of `dtype` on the host, seeded values in [-1, 2]: every intermediate of the gather is then normal or zero."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(3, h, w, generator=g) * 3 - 1).to(dtype) for h, w in sizes]


def oracle_image(img, smp, sid, num_scales, flip, P, mean, std):
    """oracle.patch_oracle.extract_patches on ((x.float().flip(...) - mean) / std) of ONE image, rows in the order of smp / sid (the
    composition of tests/image_varlen_cases.oracle_image with the float normalisation in place of transform_img)."""
    t = img.float()
    if flip[0]:
        t = t.flip(-1)
    if flip[1]:
        t = t.flip(-2)
    t = (t - torch.tensor(mean, dtype=F32).view(3, 1, 1)) / torch.tensor(std, dtype=F32).view(3, 1, 1)
    order = [np.nonzero(sid == s)[0] for s in range(num_scales)]
    deepest = max(s for s in range(num_scales) if len(order[s])) + 1
    pa, po, _ = PO.extract_patches([t], [[smp[order[s]].T.astype(np.int64)] for s in range(deepest)], P)
    back = np.argsort(np.concatenate(order[:deepest]), kind="stable")
    scales = torch.from_numpy(sid.astype(np.float32)) if num_scales > 1 else None
    return pa[0][back].contiguous(), po[0][back].contiguous(), scales


def oracle_batch(images, smp, sid, num_scales, flips, P, norm=HALF):
    outs = [oracle_image(im, s, i, num_scales, f, P, *norm) for im, s, i, f in zip(images, smp, sid, flips)]
    return tuple(torch.cat([o[k] for o in outs]) if outs[0][k] is not None else None for k in range(3))


def bits(a, b):
    """Same shape, dtype and bit pattern (NaNs included)."""
    return a.shape == b.shape and a.dtype == b.dtype == F32 and torch.equal(a.contiguous().view(I32).cpu(), b.contiguous().view(I32).cpu())


cat = lambda x: torch.from_numpy(np.concatenate(x))
on_dev = lambda images: [i.to(DEV) for i in images]


def planar(images, smp, sid, ns, flips, P, norm=HALF, **kw):
    return extract_patches_planar(images, cat(smp), [len(s) for s in smp], cat(sid) if ns > 1 else None, ns,
                                  flips=torch.tensor(flips, dtype=I32) if flips is not None else None, mean=norm[0], std=norm[1],
                                  patch_size=P, **kw)


# ---- 1: the bits of the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 8])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_element_has_the_bits_of_the_oracle(dtype, P):
    """16 x 16, 17 x 33, 37 x 53, 64 x 67 and 96 x 128 in one call (an fp16 / bf16 image behind 17 x 33 starts 2-byte aligned only), three
    levels asked for; IC.ROUNDS turns move the samples over every corner of every level and the flips over all four combinations.  Turns
    alternate between mean = std = 0.5 and the ImageNet statistics, and between the list and the flat form."""
    dt = DTYPES[dtype]
    images = make_planar(IC.SIZES, 21, dt)
    assert dt == F32 or image_tables(IC.SIZES, IC.COUNTS, 2).img_off[2] % 4 == 2
    for turn in range(IC.ROUNDS):
        smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, NS, P, 7, turn)
        flips = IC.flips_of_turn(len(images), turn)
        norm = IMAGENET if turn % 2 else HALF
        if turn % 2:
            got = planar(torch.cat([i.reshape(-1) for i in on_dev(images)]), smp, sid, NS, flips, P, norm, sizes=IC.SIZES)
        else:
            got = planar(on_dev(images), smp, sid, NS, flips, P, norm)
        want = oracle_batch(images, smp, sid, NS, flips, P, norm)
        for k, name in enumerate(("patches", "pos", "scales")):
            assert got[k].shape[0] == sum(IC.COUNTS) and bool(torch.isfinite(got[k]).all())
            assert bits(got[k], want[k]), (name, dtype, P, turn, "differs from the CPU oracle")
    # one level, no scale ids, no flips: scales is None
    smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, 1, P, 9)
    got = planar(on_dev(images), smp, sid, 1, None, P, IMAGENET)
    want = oracle_batch(images, smp, sid, 1, [(0, 0)] * len(images), P, IMAGENET)
    assert got[2] is None and bits(got[0], want[0]) and bits(got[1], want[1])
    # the reference's IndexError for a sample outside ITS image, with nothing launched
    if P == 16:
        bad = [s.copy() for s in smp]
        bad[0][0] = (1, 0)                                            # the 16 x 16 image has the one position (0, 0)
        with pytest.raises(IndexError):
            planar(on_dev(images), bad, sid, 1, None, P)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_non_finite_pixels_reach_exactly_the_elements_the_oracle_makes_non_finite(dtype):
    """A NaN, a +inf and a -inf pixel in each image (the two infinities side by side in one image: a pooled level sums them to NaN): the
    output is non-finite in exactly the oracle's elements, and every other element has its bits."""
    dt, P = DTYPES[dtype], 16
    images = make_planar(IC.SIZES, 22, dt)
    rs = np.random.RandomState(3)
    for k, im in enumerate(images):
        h, w = im.shape[1:]
        for v in (float("nan"), float("inf"), float("-inf")):
            im[rs.randint(3), rs.randint(h), rs.randint(w)] = v
        im[1, h // 2, w // 2], im[1, h // 2, w // 2 - 1] = float("inf"), float("-inf")
    hit = 0
    for turn in (0, 1, 3):
        smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, NS, P, 7, turn)
        flips = IC.flips_of_turn(len(images), turn)
        got = planar(on_dev(images), smp, sid, NS, flips, P, IMAGENET)[0].cpu()
        want = oracle_batch(images, smp, sid, NS, flips, P, IMAGENET)[0]
        bad = ~torch.isfinite(want)
        assert torch.equal(~torch.isfinite(got), bad), (dtype, turn)
        assert torch.equal(got[~bad], want[~bad]), (dtype, turn)
        hit += int(bad.sum())
    assert hit > 0, "no sampled patch held a non-finite pixel: the case shows nothing"


# ---- 2: the bits of the u8 path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 8])
def test_a_float_copy_of_a_uint8_image_has_the_bits_of_the_u8_gather(P):
    """x = u8 / 255 in fp32 CHW (an IEEE division, made on the host) gives what extract_patches_varlen gives on the bytes: the two kernels
    state one arithmetic.  The whole catalogue, flips and levels."""
    u8 = IC.make_images(IC.SIZES, 11)
    as_f32 = [torch.from_numpy(im).float().div(255).permute(2, 0, 1).contiguous() for im in u8]
    for turn in range(IC.ROUNDS):
        smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, NS, P, 7, turn)
        flips = IC.flips_of_turn(len(u8), turn)
        norm = IMAGENET if turn % 2 else HALF
        got = planar(on_dev(as_f32), smp, sid, NS, flips, P, norm)
        want = extract_patches_varlen([torch.from_numpy(im).to(DEV) for im in u8], cat(smp), IC.COUNTS, cat(sid), NS,
                                      flips=torch.tensor(flips, dtype=I32), mean=norm[0], std=norm[1], patch_size=P)
        for k in range(3):
            assert bits(got[k], want[k]) and bool(torch.isfinite(got[k]).all()), (k, turn)


# ---- 3: batch forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_batch_list_and_flat_forms_give_the_same_bits_and_every_image_those_of_the_call_on_it_alone(dtype):
    dt, P = DTYPES[dtype], 16
    # one (NI, 3, H, W) tensor, used in place: 37 x 53 has an odd element count per image
    size, n = (37, 53), 4
    batch = torch.stack(make_planar([size] * n, 31, dt)).to(DEV)
    smp, sid = IC.make_samples([size] * n, [5] * n, NS, P, 7, 2)
    flips = IC.flips_of_turn(n, 1)
    a = planar(batch, smp, sid, NS, flips, P)
    b = planar(list(batch.unbind(0)), smp, sid, NS, flips, P)
    c = planar(batch.reshape(-1), smp, sid, NS, flips, P, sizes=[size] * n)
    want = oracle_batch(list(batch.cpu().unbind(0)), smp, sid, NS, flips, P)
    for k in range(3):
        assert bits(a[k], b[k]) and bits(a[k], c[k]) and bits(a[k], want[k]), (k, dtype)
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        planar(batch.to(memory_format=torch.channels_last), smp, sid, NS, flips, P)
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        planar(batch[..., ::2], smp, sid, NS, flips, P)
    # five sizes in one call, in another order too: every image keeps the bits of the call on it alone
    images = on_dev(make_planar(IC.SIZES, 32, dt))
    smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, NS, P, 7, 1)
    flips = IC.flips_of_turn(len(images), 2)
    whole = planar(images, smp, sid, NS, flips, P, IMAGENET)
    alone = [planar([images[i]], [smp[i]], [sid[i]], NS, [flips[i]], P, IMAGENET) for i in range(len(images))]
    for k in range(3):
        assert bits(whole[k], torch.cat([o[k] for o in alone])), (k, dtype)
    perm = [3, 0, 4, 2, 1]
    pick = lambda x: [x[i] for i in perm]
    moved = planar(pick(images), pick(smp), pick(sid), NS, pick(flips), P, IMAGENET)
    for k in range(3):
        assert bits(moved[k], torch.cat([alone[i][k] for i in perm])), (k, dtype)


# ---- 4: footprint and refusals of the entry ----------------------------------------------------------------------------------------------
class Entry:
    """vtq_k_gather_patches_planar on a guard-band arena.  The images lie in one buffer with a GAP in front of every image but the first --
    one element after the first image, so that an fp16 / bf16 image starts 2-byte aligned only, more after the others -- registered as
    holes: filled with each pattern and never to be written or to reach an output.  Every table and output has the header's extent."""

    def __init__(self, dtype, P, turn=1):
        self.P, self.dt = P, dtype
        elem = self.elem = torch.empty((), dtype=dtype).element_size()
        self.images = make_planar(IC.SIZES, 41, dtype)
        self.smp, self.sid = IC.make_samples(IC.SIZES, IC.COUNTS, NS, P, 7, turn)
        self.flips = IC.flips_of_turn(len(self.images), turn)
        t = self.t = image_tables(IC.SIZES, IC.COUNTS, elem)
        gaps = np.array([0, 1, 3, 64, 7], np.int64) * elem
        self.off = t.img_off + np.cumsum(gaps)
        self.nbytes = int(t.image_bytes + gaps.sum())
        self.tab = t.tab.copy()
        self.tab[:, :2] = self.off.astype("<i8").view("<i4").reshape(-1, 2)
        NI, T = len(IC.SIZES), t.total
        specs = [("images", (self.nbytes,), U8), ("tab", (NI, 4), I32), ("patch_img", (T,), I32), ("samples", (T, 2), I32),
                 ("scale_ids", (T,), I32), ("flips", (NI, 2), I32), ("patches", (T, 3, P, P), F32), ("pos", (T, 2), F32), ("scales", (T,), F32)]
        self.arena = Arena(arena_bytes([s[1:] for s in specs]), DEV)
        self.b = {name: self.arena.carve(name, shape, dt) for name, shape, dt in specs}
        put = lambda name, a: self.b[name].copy_(torch.from_numpy(np.ascontiguousarray(a)).view(self.b[name].shape))
        end = 0
        for k, (im, o) in enumerate(zip(self.images, self.off.tolist())):
            self.arena.hole("images", f"gap {k}", end, o - end)
            raw = im.contiguous().view(-1).view(U8)
            self.b["images"][o:o + raw.numel()].copy_(raw)
            end = o + raw.numel()
        assert end == self.nbytes and (elem == 4 or self.off[1] % 4 == 2)
        put("tab", self.tab), put("patch_img", t.patch_img), put("samples", np.concatenate(self.smp)), put("scale_ids", np.concatenate(self.sid))
        put("flips", np.asarray(self.flips, np.int32))
        self.f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
        torch.cuda.synchronize()

    def outputs(self):
        return [self.b["patches"], self.b["pos"], self.b["scales"]]

    def call(self, **kw):
        t, b = self.t, self.b
        a = dict(images=b["images"].data_ptr(), image_bytes=self.nbytes, dtype=CODE[self.dt], tab=b["tab"].data_ptr(),
                 patch_img=b["patch_img"].data_ptr(), img_off=self.off, H=t.H, W=t.W, row0=t.row0, NI=len(t.H), samples=b["samples"].data_ptr(),
                 scale_ids=b["scale_ids"].data_ptr(), flips=b["flips"].data_ptr(), mean=self.f3, std=self.f3, patches=b["patches"].data_ptr(),
                 pos=b["pos"].data_ptr(), scales=b["scales"].data_ptr(), P=self.P, ns=NS)
        a.update(kw)
        host = lambda k, ty: np.ascontiguousarray(a[k]).ctypes.data_as(C.POINTER(ty)) if a[k] is not None else None
        lib = _lib.load()
        rc = lib.vtq_k_gather_patches_planar(a["images"], a["image_bytes"], a["dtype"], a["tab"], a["patch_img"], host("img_off", C.c_int64),
                                             host("H", C.c_int32), host("W", C.c_int32), host("row0", C.c_int32), a["NI"], a["samples"],
                                             a["scale_ids"], a["flips"], a["mean"], a["std"], a["patches"], a["pos"], a["scales"], a["P"],
                                             a["ns"], torch.cuda.current_stream().cuda_stream)
        return rc, lib.vtq_last_error().decode()

    def oracle(self):
        return oracle_batch(self.images, self.smp, self.sid, NS, self.flips, self.P)


@pytest.mark.parametrize("P", [16, 8])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_entry_footprint(dtype, P):
    """Guards and the gaps between the images filled with 0x00, then 0xFF (NaN in every float format): no guard byte changes, the outputs
    are bit-identical across the fills -- a byte read outside an image would be another pixel -- and equal the oracle."""
    e = Entry(DTYPES[dtype], P)

    def launch():
        rc, msg = e.call()
        assert rc == 0, msg

    got = e.arena.run_twice(launch, e.outputs)
    for g, o in zip(got, e.oracle()):
        assert bits(g, o)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_entry_refusals_leave_every_buffer_and_guard_untouched(dtype):
    e = Entry(DTYPES[dtype], 16)
    for out in e.outputs():
        e.arena.fill(out, 0xFF)
    e.arena.fill_guards(0x00)
    torch.cuda.synchronize()
    before = e.arena.mem.clone()
    i32 = lambda *v: np.array(v, np.int32)
    odd = e.off.copy()
    odd[2] += 1                                                       # not a multiple of the element size
    cases = {k: {k: None} for k in ("images", "tab", "patch_img", "img_off", "H", "W", "row0", "samples", "mean", "std", "patches", "pos")}
    cases.update({
        "NI < 1": dict(NI=0), "row0 decreases": dict(row0=i32(0, 1, 3, 2, 17, 77)), "P": dict(P=12), "num_scales 0": dict(ns=0),
        "num_scales 5": dict(ns=5), "scale_ids NULL with levels": dict(scale_ids=None),
        "an image smaller than P": dict(ns=1, scale_ids=None, H=i32(15, 17, 37, 64, 96)),
        "image leaves the buffer": dict(image_bytes=e.nbytes - 1), "unknown dtype": dict(dtype=3),
        "offset not a multiple of the element size": dict(img_off=odd)})
    for name, kw in cases.items():
        rc, msg = e.call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_gather_patches_planar:"), (name, rc, msg)
    torch.cuda.synchronize()
    assert e.arena.violations(0x00) == []
    assert torch.equal(e.arena.mem, before), "a refused call wrote to the device"
    rc, msg = e.call()                                                # and the entry still works
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bits(e.b["patches"], e.oracle()[0])


# ---- 5: end to end -----------------------------------------------------------------------------------------------------------------------
PIPE_SIZES = [(48, 64), (96, 128), (80, 80), (37, 53)]
SEED = 5


@functools.lru_cache(maxsize=None)
def _model(nscales):
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_scales=nscales if nscales > 1 else 0, pretrained=False))
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 3).items()})
    return m.to(DEV).eval()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and bool(torch.isfinite(a).all())


def _pairs(dtype, mix, seed):
    """(refs, dists): lists of (3, H, W) images in [0, 1] of `dtype` on the device; the distorted image is its reference plus noise."""
    g = torch.Generator().manual_seed(seed)
    refs = [torch.rand(3, *PIPE_SIZES[k], generator=g) for k in mix]
    dists = [(r + 0.1 * torch.randn(r.shape, generator=g)).clamp(0, 1) for r in refs]
    return [r.to(dtype).to(DEV) for r in refs], [d.to(dtype).to(DEV) for d in dists]


def _modelled(images, counts, keys, nscales, seed=SEED):
    """extract_patches_planar at the coordinates of the sampler's numpy restatement for (seed, key, size, count)."""
    sizes = [tuple(i.shape[1:]) for i in images]
    smp, sid, lengths = SM.batch(sizes, counts, keys, seed, nscales)
    out = extract_patches_planar(images, torch.from_numpy(smp), lengths, torch.from_numpy(sid) if nscales > 1 else None, nscales)
    return out, lengths, smp


def _direct(m, refs, dists, counts, kr, kd, nscales):
    (pr, qr, sr), lens, smp_r = _modelled(refs, counts, kr, nscales)
    (pd, qd, sd), _, smp_d = _modelled(dists, counts, kd, nscales)
    with torch.no_grad():
        return m.forward_varlen((pr, pd), (qr, qd), (sr, sd), lens)[0], smp_r, smp_d


@pytest.mark.parametrize("nscales", [1, 3])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_metric_has_the_bits_of_forward_varlen_at_the_modelled_coordinates(dtype, nscales):
    """Four pairs of four sizes (37 x 53 among them) with 20 .. 45 patches: the list form, aligned and not; then a (B, 3, H, W) batch
    tensor.  keys=None draws from the call counter: another call, other scores; the same keys again, the same bits."""
    m, dt = _model(nscales), DTYPES[dtype]
    refs, dists = _pairs(dt, [0, 1, 2, 3], 50)
    counts, keys = [20, 45, 31, 24], [11, 2 ** 63 + 5, 13, 14]
    metric = ImageMetric(m, patch_count=counts, num_scales=nscales, seed=SEED)
    q = metric(refs, dists, keys=keys)
    want, smp_r, smp_d = _direct(m, refs, dists, counts, keys, keys, nscales)
    torch.cuda.synchronize()
    assert q.shape == (4,) and same(q, want) and np.array_equal(smp_r, smp_d)
    # unaligned: 2B keys, two coordinate sets, pairs of two sizes
    mixed = dists[1:] + dists[:1]
    keys2 = keys + [21, 22, 23, 24]
    q2 = metric(refs, mixed, keys=keys2, aligned=False)
    want2, smp_r, smp_d = _direct(m, refs, mixed, counts, keys2[:4], keys2[4:], nscales)
    torch.cuda.synchronize()
    assert same(q2, want2) and not np.array_equal(smp_r, smp_d)
    with pytest.raises(ValueError, match="aligned sampling"):
        metric(refs, mixed, keys=keys)
    assert metric.count == 2, "a refused call was counted"
    # one batch tensor per side, used in place; one patch count for all
    B = 3
    rb = torch.stack(_pairs(dt, [1] * B, 51)[0])
    db = (rb.float() * 0.9).to(dt)
    mb = ImageMetric(m, patch_count=40, num_scales=nscales, seed=SEED)
    qb = mb(rb, db, keys=[7, 8, 9])
    wantb, _, _ = _direct(m, list(rb.unbind(0)), list(db.unbind(0)), [40] * B, [7, 8, 9], [7, 8, 9], nscales)
    a, b = mb(rb, db), mb(rb, db)                                     # keys from the call counter
    again = mb(rb, db, keys=[7, 8, 9])
    torch.cuda.synchronize()
    assert same(qb, wantb) and same(again, qb) and not torch.equal(a, b) and mb.count == 4


@pytest.mark.parametrize("nscales", [1, 3])
def test_uint8_device_images_have_the_bits_of_submit_images(nscales):
    """The same images as host arrays through ImagePairVarlenPipeline.submit_images, with the same keys and seed: lists of two sizes,
    aligned and not, then a (B, H, W, 3) batch tensor against the list of its images; also with three repeats."""
    m = _model(nscales)
    rs = np.random.RandomState(60)
    refs = [rs.randint(0, 256, size=(*PIPE_SIZES[k], 3), dtype=np.uint8) for k in (0, 1, 3)]
    dists = [rs.randint(0, 256, size=r.shape, dtype=np.uint8) for r in refs]
    dev = lambda x: [torch.from_numpy(i).to(DEV) for i in x]
    cap = dict(max_pairs=9, max_image_bytes=4 * 3 * 96 * 128, max_patches=3 * 3 * 45, num_scales=nscales)
    counts, keys = [20, 45, 31], [3, 4, 5]
    for R in (1, 3):
        pipe = ImagePairVarlenPipeline(m, **cap)
        metric = ImageMetric(m, patch_count=counts, num_scales=nscales, num_repeats=R, seed=SEED)
        want = pipe.submit_images(refs, dists, counts, keys=keys, seed=SEED, num_repeats=R)
        got = metric(dev(refs), dev(dists), keys=keys)
        want2 = pipe.submit_images(refs, dists[::-1], counts, keys=keys + [6, 7, 8], seed=SEED, aligned=False, num_repeats=R)
        got2 = metric(dev(refs), dev(dists[::-1]), keys=keys + [6, 7, 8], aligned=False)
        torch.cuda.synchronize()
        assert got.shape == (3,) and got.dtype == (torch.float64 if R > 1 else F32)
        assert same(got, want) and same(got2, want2), R
    same_size = [refs[1], dists[1]]
    batch = torch.from_numpy(np.stack(same_size)).to(DEV)
    metric = ImageMetric(m, patch_count=33, num_scales=nscales, seed=SEED)
    got = metric(batch, batch.flip(0), keys=[1, 2])
    want = ImagePairVarlenPipeline(m, **cap).submit_images(same_size, same_size[::-1], 33, keys=[1, 2], seed=SEED)
    torch.cuda.synchronize()
    assert same(got, want)


@pytest.mark.parametrize("nscales", [1, 3])
def test_uint8_device_images_with_the_weighted_sampler_have_the_bits_of_submit_images(nscales):
    """sampler=WeightedPatchSampler(diff_weight > 0) on uint8 device images is sampling.sample_patches_weighted: the scores of
    submit_images with that sampler on the same images as host arrays, aligned and not, one repeat and two."""
    from vtamiq_amd.sampling import WeightedPatchSampler
    m = _model(nscales)
    rs = np.random.RandomState(61)
    refs = [rs.randint(0, 256, size=(*PIPE_SIZES[k], 3), dtype=np.uint8) for k in (0, 1, 3)]
    dists = [r.copy() for r in refs]
    for d in dists:                                                   # the pair differs in one corner: the weights are not uniform
        d[:d.shape[0] // 2, :d.shape[1] // 3] = rs.randint(0, 256, size=d[:d.shape[0] // 2, :d.shape[1] // 3].shape, dtype=np.uint8)
    dev = lambda x: [torch.from_numpy(i).to(DEV) for i in x]
    cap = dict(max_pairs=6, max_image_bytes=4 * 3 * 96 * 128, max_patches=2 * 3 * 45, num_scales=nscales)
    counts, keys = [20, 45, 31], [3, 4, 5]
    sampler = WeightedPatchSampler(diff_weight=1.0, uniform_weight=0.1)
    for R in (1, 2):
        pipe = ImagePairVarlenPipeline(m, **cap)
        metric = ImageMetric(m, patch_count=counts, num_scales=nscales, num_repeats=R, seed=SEED, sampler=sampler)
        want = pipe.submit_images(refs, dists, counts, keys=keys, seed=SEED, num_repeats=R, sampler=sampler)
        got = metric(dev(refs), dev(dists), keys=keys)
        want2 = pipe.submit_images(refs, dists, counts, keys=keys + [6, 7, 8], seed=SEED, aligned=False, num_repeats=R, sampler=sampler)
        got2 = metric(dev(refs), dev(dists), keys=keys + [6, 7, 8], aligned=False)
        torch.cuda.synchronize()
        assert same(got, want) and same(got2, want2) and not torch.equal(got, got2), R
    plain = ImageMetric(m, patch_count=counts, num_scales=nscales, seed=SEED)(dev(refs), dev(dists), keys=keys)
    assert not torch.equal(plain, ImageMetric(m, patch_count=counts, num_scales=nscales, seed=SEED, sampler=sampler)(dev(refs), dev(dists), keys=keys))
    with pytest.raises(NotImplementedError, match="defined on bytes"):
        ImageMetric(m, sampler=sampler)(*_pairs(F32, [0], 1))


@pytest.mark.parametrize("nscales", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_group_has_the_bits_of_forward_group_at_the_modelled_coordinates(dtype, nscales):
    """G = 2 references of two sizes, M = 5 distorted images of sizes and patch counts of their own."""
    m, dt = _model(nscales), DTYPES[dtype]
    refs, _ = _pairs(dt, [0, 1], 70)
    dists, _ = _pairs(dt, [0, 1, 2, 1, 3], 71)
    index, cr, cd, keys = [0, 1, 1, 0, 1], [33, 45], [33, 20, 41, 45, 25], list(range(100, 107))
    metric = ImageMetric(m, patch_count=cr, num_scales=nscales, seed=SEED)
    q = metric.group(refs, dists, index, keys=keys, patch_count_dist=cd)
    (pr, qr, sr), lr, _ = _modelled(refs, cr, keys[:2], nscales)
    (pd, qd, sd), ld, _ = _modelled(dists, cd, keys[2:], nscales)
    with torch.no_grad():
        want = m.forward_group((pr, pd), (qr, qd), (sr, sd), index, lengths=(lr, ld))[0]
    torch.cuda.synchronize()
    assert q.shape == (5,) and same(q, want)
    with pytest.raises(ValueError, match="ref_index"):
        metric.group(refs, dists, [0, 1, 2, 0, 1], keys=keys, patch_count_dist=cd)
    # three repeats: the mean of the three single calls with repeat_key, for the group and for pairs
    rep = ImageMetric(m, patch_count=cr, num_scales=nscales, num_repeats=3, seed=SEED)
    got = rep.group(refs, dists, index, keys=keys, patch_count_dist=cd)
    singles = [metric.group(refs, dists, index, keys=[repeat_key(k, r) for k in keys], patch_count_dist=cd) for r in range(3)]
    assert same(singles[0], q)
    want = average_over_repeats(torch.cat(singles), 3)
    pr_, pd_ = _pairs(dt, [2, 3], 72)
    got_p = ImageMetric(m, patch_count=30, num_scales=nscales, num_repeats=3, seed=SEED)(pr_, pd_, keys=[8, 9])
    one = ImageMetric(m, patch_count=30, num_scales=nscales, seed=SEED)
    want_p = average_over_repeats(torch.cat([one(pr_, pd_, keys=[repeat_key(k, r) for k in (8, 9)]) for r in range(3)]), 3)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and same(got, want) and got_p.shape == (2,) and same(got_p, want_p)


def test_metric_on_a_side_stream_and_between_two_forwards():
    """The same calls with a side stream current while the default stream is busy have the bits of the default-stream calls; a forward
    before and after a metric call keeps its bits (the metric leaves nothing behind in the engine)."""
    nscales = 3
    m = _model(nscales)
    refs, dists = _pairs(F16, [0, 1, 2, 3], 80)
    grefs, gdists = _pairs(F32, [1, 3], 81)[0], _pairs(F32, [3, 1, 0], 82)[0]

    def run():
        metric = ImageMetric(m, patch_count=[25, 40, 31, 22], num_scales=nscales, seed=SEED, num_repeats=2)
        group = ImageMetric(m, patch_count=28, num_scales=nscales, seed=SEED)
        return [metric(refs, dists), metric(refs, dists[::-1], aligned=False), group.group(grefs, gdists, [0, 1, 1]), metric(refs, dists)]

    spec = m.spec
    p, pos, sc = (torch.from_numpy(x).to(DEV) for x in synth.make_inputs(spec, 2, 24, 9))        # collated: [B, 2, ...]
    args = tuple((x[:, 0].contiguous(), x[:, 1].contiguous()) for x in (p, pos, sc))
    with torch.no_grad():
        before = m(*args)[0].clone()
    want = run()
    with torch.no_grad():
        after = m(*args)[0].clone()
    side, busy = torch.cuda.Stream(), Busy()
    torch.cuda.synchronize()
    busy(torch.cuda.default_stream())
    with torch.cuda.stream(side):
        got = run()
    torch.cuda.synchronize()
    assert same(before, after)
    for g, w in zip(got, want):
        assert same(g, w)
    assert not torch.equal(want[0], want[3])
