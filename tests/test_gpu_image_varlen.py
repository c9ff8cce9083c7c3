"""The image front end for images of different sizes on the GPU: vtq_k_gather_patches_u8 (include/vtamiq_hip_images.h),
vtamiq_amd.patches.extract_patches_varlen and vtamiq_amd.pipeline.ImagePairVarlenPipeline.

The contract every test turns on: an image's patches have the BITS extract_patches gives for that image alone -- whatever else is in the
batch, wherever the image starts in the byte buffer -- and the pipeline's scores the bits of forward_varlen / forward_group(lengths=) on those.
The CPU oracle beside the bit checks keeps them from being vacuous."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import image_varlen_cases as IC
from tests.footprint import Arena, arena_bytes
from tests.test_gpu_streams import Busy
from vtamiq_amd import VTAMIQ, _lib, synth
from vtamiq_amd.patches import extract_patches, extract_patches_varlen, image_tables
from vtamiq_amd.pipeline import ImagePairVarlenPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def alone(img, smp, sid, num_scales, flip, P):
    """extract_patches on ONE image with the levels that image can hold: (patches (n, 3, P, P), pos (n, 2), scales (n,) | None)."""
    h, w = img.shape[:2]
    ns = len(IC.levels_with_a_patch(h, w, num_scales, P))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pa, po, sc = extract_patches(dev(img)[None], dev(smp)[None], dev(sid)[None] if ns > 1 else None, ns,
                                 flips=dev(np.asarray([flip], np.int32)), patch_size=P)
    if num_scales > 1 and sc is None:
        sc = torch.zeros(1, smp.shape[0], device=DEV)                 # one level: every id is 0
    return pa[0], po[0], (sc[0] if num_scales > 1 else None)


def alone_batch(images, smp, sid, num_scales, flips, P):
    outs = [alone(im, s, i, num_scales, f, P) for im, s, i, f in zip(images, smp, sid, flips)]
    return tuple(torch.cat([o[k] for o in outs]) if outs[0][k] is not None else None for k in range(3))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 1: the bits of the image alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 8])
def test_every_image_has_the_bits_of_extract_patches_on_it_alone(P):
    """One call over 16 x 16, 17 x 33, 37 x 53, 64 x 67 and 96 x 128 packed back to back (odd offsets), 1, 2, 5, 9 and 60 patches, three
    levels asked for (each image uses those it can hold).  IC.ROUNDS turns move the samples over every corner of every level and the flips
    over all four combinations (tests/test_image_varlen_layout.py checks that they do)."""
    ns = IC.NUM_SCALES
    images = IC.make_images(IC.SIZES, 11)
    assert any(o % 2 for o in image_tables(IC.SIZES, IC.COUNTS).img_off)
    row0 = np.concatenate([[0], np.cumsum(IC.COUNTS)])
    perm = [3, 0, 4, 2, 1]
    pick = lambda x: [x[i] for i in perm]
    rows = torch.from_numpy(np.concatenate([np.arange(row0[i], row0[i + 1]) for i in perm])).to(DEV)
    for turn in range(IC.ROUNDS):
        smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, ns, P, 7, turn)
        flips = IC.flips_of_turn(len(images), turn)
        dev_images = [torch.from_numpy(im).to(DEV) for im in images]
        cat = lambda x: torch.from_numpy(np.concatenate(x))
        if turn % 2:                                                  # the flat form, host samples
            got = extract_patches_varlen(torch.cat([i.reshape(-1) for i in dev_images]), cat(smp), IC.COUNTS, cat(sid), ns,
                                         flips=torch.tensor(flips, dtype=I32), patch_size=P, sizes=IC.SIZES)
        else:                                                         # the list form, device samples
            got = extract_patches_varlen(dev_images, cat(smp).to(DEV), IC.COUNTS, cat(sid).to(DEV), ns,
                                         flips=torch.tensor(flips, dtype=I32, device=DEV), patch_size=P)
        want = alone_batch(images, smp, sid, ns, flips, P)
        oracle = IC.oracle_batch(images, smp, sid, ns, flips, P)
        for k, name in enumerate(("patches", "pos", "scales")):
            assert got[k].shape[0] == sum(IC.COUNTS) and got[k].dtype == F32
            assert same(got[k], want[k]), (name, turn, "differs from extract_patches on the image alone")
            assert torch.equal(got[k].cpu(), oracle[k]), (name, turn, "differs from the CPU oracle")
        # the images in another order: the same bits in that order
        moved = extract_patches_varlen(pick(dev_images), cat(pick(smp)), pick(IC.COUNTS), cat(pick(sid)), ns,
                                       flips=torch.tensor(pick(flips), dtype=I32), patch_size=P)
        for k in range(3):
            assert same(moved[k], got[k][rows]), (k, turn)
    # one level, no scale ids, no flips: scales is None
    smp, sid = IC.make_samples(IC.SIZES, IC.COUNTS, 1, P, 9)
    got = extract_patches_varlen([torch.from_numpy(im).to(DEV) for im in images], torch.from_numpy(np.concatenate(smp)), IC.COUNTS, patch_size=P)
    want = alone_batch(images, smp, sid, 1, [(0, 0)] * len(images), P)
    assert got[2] is None and same(got[0], want[0]) and same(got[1], want[1])
    # the reference's IndexError for a sample outside ITS image (inside a larger one of the batch), with nothing launched
    bad = np.concatenate(smp)
    bad[0] = (1, 0)                                                   # the 16 x 16 image has the one position (0, 0) at P = 16
    if P == 16:
        with pytest.raises(IndexError):
            extract_patches_varlen([torch.from_numpy(im).to(DEV) for im in images], torch.from_numpy(bad), IC.COUNTS, patch_size=P)


# ---- 2, 3: footprint and refusals of the entry -------------------------------------------------------------------------------------------
class Entry:
    """vtq_k_gather_patches_u8 on a guard-band arena: the image buffer has exactly sum 3 H W bytes, every table and output the header's extent."""

    def __init__(self, P, turn=1):
        self.P, self.ns = P, IC.NUM_SCALES
        self.images = IC.make_images(IC.SIZES, 11)
        self.smp, self.sid = IC.make_samples(IC.SIZES, IC.COUNTS, self.ns, P, 7, turn)
        self.flips = IC.flips_of_turn(len(self.images), turn)
        t = self.t = image_tables(IC.SIZES, IC.COUNTS)
        NI, T = len(IC.SIZES), t.total
        specs = [("images", (t.image_bytes,), U8), ("tab", (NI, 4), I32), ("patch_img", (T,), I32), ("samples", (T, 2), I32),
                 ("scale_ids", (T,), I32), ("flips", (NI, 2), I32), ("patches", (T, 3, P, P), F32), ("pos", (T, 2), F32), ("scales", (T,), F32)]
        self.arena = Arena(arena_bytes([s[1:] for s in specs]), DEV)
        self.b = {name: self.arena.carve(name, shape, dtype) for name, shape, dtype in specs}
        put = lambda name, a: self.b[name].copy_(torch.from_numpy(np.ascontiguousarray(a)).view(self.b[name].shape))
        put("images", np.concatenate([im.reshape(-1) for im in self.images]))
        put("tab", t.tab), put("patch_img", t.patch_img), put("samples", np.concatenate(self.smp)), put("scale_ids", np.concatenate(self.sid))
        put("flips", np.asarray(self.flips, np.int32))
        self.f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
        torch.cuda.synchronize()

    def outputs(self):
        return [self.b["patches"], self.b["pos"], self.b["scales"]]

    def call(self, **kw):
        t, b = self.t, self.b
        a = dict(images=b["images"].data_ptr(), image_bytes=t.image_bytes, tab=b["tab"].data_ptr(), patch_img=b["patch_img"].data_ptr(),
                 img_off=t.img_off, H=t.H, W=t.W, row0=t.row0, NI=len(t.H), samples=b["samples"].data_ptr(),
                 scale_ids=b["scale_ids"].data_ptr(), flips=b["flips"].data_ptr(), mean=self.f3, std=self.f3, patches=b["patches"].data_ptr(),
                 pos=b["pos"].data_ptr(), scales=b["scales"].data_ptr(), P=self.P, ns=self.ns)
        a.update(kw)
        host = lambda k, ty: a[k].ctypes.data_as(C.POINTER(ty)) if a[k] is not None else None
        lib = _lib.load()
        rc = lib.vtq_k_gather_patches_u8(a["images"], a["image_bytes"], a["tab"], a["patch_img"], host("img_off", C.c_int64), host("H", C.c_int32),
                                         host("W", C.c_int32), host("row0", C.c_int32), a["NI"], a["samples"], a["scale_ids"], a["flips"],
                                         a["mean"], a["std"], a["patches"], a["pos"], a["scales"], a["P"], a["ns"],
                                         torch.cuda.current_stream().cuda_stream)
        return rc, lib.vtq_last_error().decode()


@pytest.mark.parametrize("P", [16, 8])
def test_entry_footprint(P):
    """Guards filled with 0x00, then 0xFF: no guard byte changes (the 0xFF fill would turn any byte read outside the image buffer into a
    different pixel), the outputs are bit-identical across the fills and equal the oracle."""
    e = Entry(P)

    def launch():
        rc, msg = e.call()
        assert rc == 0, msg

    got = e.arena.run_twice(launch, e.outputs)
    oracle = IC.oracle_batch(e.images, e.smp, e.sid, e.ns, e.flips, P)
    for g, o in zip(got, oracle):
        assert torch.equal(g.cpu(), o)


def test_entry_refusals_leave_every_buffer_and_guard_untouched():
    e = Entry(16)
    for out in e.outputs():
        e.arena.fill(out, 0xFF)
    e.arena.fill_guards(0x00)
    torch.cuda.synchronize()
    before = e.arena.mem.clone()
    i32 = lambda *v: np.array(v, np.int32)
    t = e.t
    cases = {k: {k: None} for k in ("images", "tab", "patch_img", "img_off", "H", "W", "row0", "samples", "mean", "std", "patches", "pos")}
    cases.update({
        "NI < 1": dict(NI=0), "row0 decreases": dict(row0=i32(0, 1, 3, 2, 17, 77)), "P": dict(P=12), "num_scales 0": dict(ns=0),
        "num_scales 5": dict(ns=5), "scale_ids NULL with levels": dict(scale_ids=None),
        "last level of a one-level call smaller than P": dict(ns=1, scale_ids=None, H=i32(15, 17, 37, 64, 96)),
        "image leaves the buffer": dict(image_bytes=t.image_bytes - 1)})
    for name, kw in cases.items():
        rc, msg = e.call(**kw)
        assert rc != 0 and msg.startswith("vtq_k_gather_patches_u8:"), (name, rc, msg)
    torch.cuda.synchronize()
    assert e.arena.violations(0x00) == []
    assert torch.equal(e.arena.mem, before), "a refused call wrote to the device"
    rc, msg = e.call()                                                # and the entry still works
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(e.b["patches"].cpu(), IC.oracle_batch(e.images, e.smp, e.sid, e.ns, e.flips, 16)[0])


# ---- 4, 5: the pipeline ------------------------------------------------------------------------------------------------------------------
PIPE_SIZES = [(48, 64), (96, 128), (80, 80)]


@functools.lru_cache(maxsize=None)
def _model(nscales):
    kw = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_scales=nscales if nscales > 1 else 0, pretrained=False))
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 3).items()})
    return m.to(DEV).eval()


def _image_and_samples(rs, size, n, nscales, P=16):
    h, w = size
    lv = IC.levels_with_a_patch(h, w, nscales, P)
    sid = np.sort(rs.randint(0, len(lv), size=n)).astype(np.int32)
    smp = np.stack([rs.randint(0, (h >> sid) - P + 1), rs.randint(0, (w >> sid) - P + 1)], axis=-1).astype(np.int32)
    return rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8), smp, sid


def _batches(nscales):
    """Five batches, each another mix of sizes and counts in 20 .. 60; the third one with unaligned sampling and pairs of two sizes."""
    rs = np.random.RandomState(5)
    mixes = [[0, 1, 2], [1, 1, 0, 2], [2, 0], [0, 2, 1, 1], [2, 2, 1]]
    out = []
    for it, mix in enumerate(mixes):
        refs, dists, smp_r, sid_r, smp_d, sid_d = [], [], [], [], [], []
        for b, k in enumerate(mix):
            n = int(rs.randint(20, 61))
            im, s, i = _image_and_samples(rs, PIPE_SIZES[k], n, nscales)
            refs.append(im), smp_r.append(s), sid_r.append(i)
            if it == 2:                                               # the distorted image has its own size and samples
                im2, s2, i2 = _image_and_samples(rs, PIPE_SIZES[(k + 1) % 3], n, nscales)
                dists.append(im2), smp_d.append(s2), sid_d.append(i2)
            else:
                dists.append(rs.randint(0, 256, size=im.shape, dtype=np.uint8))
        aligned = it != 2
        out.append((refs, dists, smp_r if aligned else smp_r + smp_d, (sid_r if aligned else sid_r + sid_d) if nscales > 1 else None))
    return out


def _direct_side(images, smp, sid, nscales):
    outs = [alone(im, s, i if i is not None else np.zeros(len(s), np.int32), nscales, (0, 0), 16) for im, s, i in zip(images, smp, sid)]
    return [o[0] for o in outs], [o[1] for o in outs], ([o[2] for o in outs] if nscales > 1 else None)


def _direct(m, batch, nscales):
    refs, dists, smp, sid = batch
    B = len(refs)
    smp2 = smp if len(smp) == 2 * B else smp + smp
    sid2 = [None] * (2 * B) if sid is None else (sid if len(sid) == 2 * B else sid + sid)
    pr, qr, sr = _direct_side(refs, smp2[:B], sid2[:B], nscales)
    pd, qd, sd = _direct_side(dists, smp2[B:], sid2[B:], nscales)
    with torch.no_grad():
        return m.forward_varlen((pr, pd), (qr, qd), (sr, sd), [len(s) for s in smp2[:B]])[0]


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("nscales", [1, 3])
def test_varlen_pipeline_matches_the_direct_path(nscales, side_stream):
    """Five batches over two slots, every batch another mix of 48 x 64, 96 x 128 and 80 x 80 images with 20 .. 60 patches: the scores equal
    forward_varlen on per-image extract_patches outputs, bit for bit -- also with a side stream current while the default stream is busy.
    An out-of-range sample raises IndexError with nothing enqueued, a batch over capacity ValueError, and the next batch is still right."""
    m = _model(nscales)
    batches = _batches(nscales)
    cap = dict(max_pairs=4, max_image_bytes=2 * 3 * (96 * 128 * 2 + 80 * 80 + 48 * 64), max_patches=4 * 60, num_scales=nscales)

    def run():
        pipe = ImagePairVarlenPipeline(m, **cap)
        got = [pipe.submit(r, d, s, scale_ids=i) for r, d, s, i in batches[:4]]
        refs, dists, smp, sid = batches[4]
        bad = [s.copy() for s in smp]
        bad[1][3, 0] = (refs[1].shape[0] >> (int(sid[1][3]) if sid is not None else 0)) - 15           # one row past its level
        count = pipe.count
        with pytest.raises(IndexError):
            pipe.submit(refs, dists, bad, scale_ids=sid)
        with pytest.raises(ValueError):                               # five pairs in a pipeline built for four
            pipe.submit(refs + refs[:2], dists + dists[:2], smp + smp[:2], scale_ids=sid + sid[:2] if sid is not None else None)
        assert pipe.count == count and pipe._batch is None, "a refused batch took a slot"
        got.append(pipe.submit(refs, dists, smp, scale_ids=sid))
        return got

    if side_stream:
        side, busy = torch.cuda.Stream(), Busy()
        torch.cuda.synchronize()
        busy(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            got = run()
    else:
        got = run()
    torch.cuda.synchronize()
    for b, q in zip(batches, got):
        want = _direct(m, b, nscales)
        torch.cuda.synchronize()
        assert q.shape == (len(b[0]),) and same(q, want)
    assert not torch.equal(got[0][:2], got[1][:2])


@pytest.mark.parametrize("nscales", [1, 3])
def test_submit_group_matches_forward_group_on_the_direct_path(nscales):
    """G = 2 references of different sizes, M = 5 distorted images of sizes and patch counts of their own: submit_group equals
    forward_group(lengths=) on per-image extract_patches outputs, bit for bit."""
    m = _model(nscales)
    rs = np.random.RandomState(17)
    ref = [_image_and_samples(rs, PIPE_SIZES[k], n, nscales) for k, n in ((0, 33), (1, 60))]
    dist = [_image_and_samples(rs, PIPE_SIZES[k], n, nscales) for k, n in ((0, 33), (1, 20), (2, 47), (1, 60), (0, 25))]
    index = [0, 1, 1, 0, 1]
    col = lambda x, k: [t[k] for t in x]
    pipe = ImagePairVarlenPipeline(m, max_pairs=4, max_image_bytes=3 * (3 * 96 * 128 + 3 * 48 * 64 + 80 * 80), max_patches=185, num_scales=nscales)
    ids = dict(scale_ids_ref=col(ref, 2), scale_ids_dist=col(dist, 2)) if nscales > 1 else {}
    q = pipe.submit_group(col(ref, 0), col(dist, 0), index, col(ref, 1), col(dist, 1), **ids)
    pr, qr, sr = _direct_side(col(ref, 0), col(ref, 1), col(ref, 2), nscales)
    pd, qd, sd = _direct_side(col(dist, 0), col(dist, 1), col(dist, 2), nscales)
    cat = lambda x: torch.cat(x) if x is not None else None
    with torch.no_grad():
        want = m.forward_group((cat(pr), cat(pd)), (cat(qr), cat(qd)), (cat(sr), cat(sd)), index,
                               lengths=([len(s) for s in col(ref, 1)], [len(s) for s in col(dist, 1)]))[0]
    torch.cuda.synchronize()
    assert q.shape == (5,) and same(q, want)
    with pytest.raises(ValueError):
        pipe.submit_group(col(ref, 0), col(dist, 0), [0, 1, 2, 0, 1], col(ref, 1), col(dist, 1), **ids)       # reference 2 of 2


# ---- 6: acquire() + launch(), entries mixed on one ring, the uniform pipeline both ways ------------------------------------------------
def _group_case(nscales):
    rs = np.random.RandomState(17)
    ref = [_image_and_samples(rs, PIPE_SIZES[k], n, nscales) for k, n in ((0, 33), (1, 60))]
    dist = [_image_and_samples(rs, PIPE_SIZES[k], n, nscales) for k, n in ((0, 33), (1, 20), (2, 47), (1, 60), (0, 25))]
    return ref, dist, [0, 1, 1, 0, 1]


def _col(x, k):
    return [t[k] for t in x]


CAP = dict(max_pairs=4, max_image_bytes=2 * 3 * (96 * 128 * 2 + 80 * 80 + 48 * 64), max_patches=4 * 60)


def _write(pinned, images, smp, sid):
    views, hs, hd = pinned
    assert len(views) == len(images) and (hd is None) == (sid is None)
    for v, im in zip(views, images):
        assert v.shape == im.shape and v.dtype == np.uint8
        v[...] = im
    hs[:] = np.concatenate(smp)
    if hd is not None:
        hd[:] = np.concatenate(sid)
    return hs


@pytest.mark.parametrize("nscales", [1, 3])
def test_acquire_and_launch_have_the_bits_of_submit(nscales):
    """The caller writes images and samples into the pinned views of acquire(): launch() equals submit() and launch_group() equals
    submit_group() of the same batch on a fresh pipeline, bit for bit.  launch() without acquire() is a RuntimeError; a sample one row past
    its level in the pinned view an IndexError that takes no slot, and the corrected view gives the right bits; sides that differ in patch
    counts are no pairs."""
    m = _model(nscales)
    cap = dict(CAP, num_scales=nscales)
    refs, dists, smp, sid = _batches(nscales)[0]
    want = ImagePairVarlenPipeline(m, **cap).submit(refs, dists, smp, scale_ids=sid)
    pipe = ImagePairVarlenPipeline(m, **cap)
    with pytest.raises(RuntimeError):
        pipe.launch()
    lens = [len(s) for s in smp]
    batch = pipe.plan([r.shape[:2] for r in refs], [d.shape[:2] for d in dists], lens, lens)
    hs = _write(pipe.acquire(batch), refs + dists, smp + smp, sid + sid if sid is not None else None)
    row = lens[0] + 3                                                 # sample 3 of the second image
    keep = int(hs[row, 0])
    hs[row, 0] = (refs[1].shape[0] >> (int(sid[1][3]) if sid is not None else 0)) - 15                 # one row past its level
    with pytest.raises(IndexError):
        pipe.launch()
    assert pipe.count == 0 and pipe._batch is batch, "a refused launch took the slot"
    hs[row, 0] = keep
    got = pipe.launch()
    assert pipe.count == 1 and pipe._batch is None
    torch.cuda.synchronize()
    assert got.shape == (len(refs),) and same(got, want)
    direct = _direct(m, (refs, dists, smp, sid), nscales)
    torch.cuda.synchronize()
    assert same(want, direct)

    ref, dist, index = _group_case(nscales)
    ids = dict(scale_ids_ref=_col(ref, 2), scale_ids_dist=_col(dist, 2)) if nscales > 1 else {}
    want = ImagePairVarlenPipeline(m, **cap).submit_group(_col(ref, 0), _col(dist, 0), index, _col(ref, 1), _col(dist, 1), **ids)
    both = ref + dist
    batch = pipe.plan([t[0].shape[:2] for t in ref], [t[0].shape[:2] for t in dist], [len(t[1]) for t in ref], [len(t[1]) for t in dist])
    _write(pipe.acquire(batch), _col(both, 0), _col(both, 1), _col(both, 2) if nscales > 1 else None)
    with pytest.raises(ValueError):                                   # 2 references and 5 distorted images are no pairs
        pipe.launch()
    assert pipe.count == 1 and pipe._batch is batch
    got = pipe.launch_group(index)
    torch.cuda.synchronize()
    assert got.shape == (5,) and same(got, want) and pipe.count == 2

    pipe.acquire(pipe.plan([(48, 64), (80, 80)], [(48, 64), (80, 80)], [20, 30], [20, 31]))
    with pytest.raises(ValueError):                                   # as many images on both sides, other patch counts
        pipe.launch()
    assert pipe.count == 2


def _mixed_calls(nscales):
    """Seven calls cycling through the four entries, each another layout of a slot's block; the keys are given, so that a result does
    not depend on the pipeline's submission counter."""
    b = _batches(nscales)
    ref, dist, index = _group_case(nscales)
    ids = dict(scale_ids_ref=_col(ref, 2), scale_ids_dist=_col(dist, 2)) if nscales > 1 else {}
    ids2 = dict(scale_ids_ref=_col(ref, 2)[::-1], scale_ids_dist=_col(dist, 2)[:3]) if nscales > 1 else {}
    return [
        lambda p: p.submit(b[0][0], b[0][1], b[0][2], scale_ids=b[0][3]),
        lambda p: p.submit_images(b[1][0], b[1][1], 30, keys=[11, 12, 13, 14], seed=5),
        lambda p: p.submit_group(_col(ref, 0), _col(dist, 0), index, _col(ref, 1), _col(dist, 1), **ids),
        lambda p: p.submit_group_images(_col(ref, 0), _col(dist, 0), index, [33, 60], keys=list(range(100, 107)), seed=5,
                                        patch_count_dist=[33, 20, 47, 60, 25]),
        lambda p: p.submit(b[2][0], b[2][1], b[2][2], scale_ids=b[2][3]),                               # unaligned: 2B sample arrays
        lambda p: p.submit_images(b[3][0], b[3][1], [25, 40, 31, 52], keys=[2 ** 63 + 1, 22, 23, 24], seed=6),
        lambda p: p.submit_group(_col(ref, 0)[::-1], _col(dist, 0)[:3], [1, 0, 0], _col(ref, 1)[::-1], _col(dist, 1)[:3], **ids2),
    ]


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("nscales", [1, 3])
def test_entries_mixed_on_one_ring_have_the_bits_of_a_fresh_pipeline(nscales, depth, side_stream):
    """submit, submit_images, submit_group, submit_group_images in turn on ONE pipeline: every slot is reused by a batch of another layout
    (host-sampled: the whole block is uploaded; device-sampled: its front, the rest is written by the sampler).  Each result equals the
    same call on a pipeline of its own; a batch refused in the middle (five pairs into max_pairs=4) takes no slot and the calls behind
    it are still right.  Also with a side stream current while the default stream is busy."""
    m = _model(nscales)
    cap = dict(CAP, num_scales=nscales, depth=depth)
    calls = _mixed_calls(nscales)
    refs, dists, smp, sid = _batches(nscales)[4]

    def run():
        pipe = ImagePairVarlenPipeline(m, **cap)
        got = []
        for i, call in enumerate(calls):
            if i == 4:
                with pytest.raises(ValueError):
                    pipe.submit(refs + refs[:2], dists + dists[:2], smp + smp[:2], scale_ids=sid + sid[:2] if sid is not None else None)
                assert pipe.count == 4 and pipe._batch is None, "a refused batch took a slot"
            got.append(call(pipe))
        assert pipe.count == len(calls)
        return got

    if side_stream:
        side, busy = torch.cuda.Stream(), Busy()
        torch.cuda.synchronize()
        busy(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            got = run()
    else:
        got = run()
    torch.cuda.synchronize()
    for i, (call, g) in enumerate(zip(calls, got)):
        want = call(ImagePairVarlenPipeline(m, **cap))
        torch.cuda.synchronize()
        assert same(g, want), i
    assert [g.shape[0] for g in got] == [3, 4, 5, 5, 2, 4, 3]


@pytest.mark.parametrize("nscales,size", [(1, (48, 64)), (3, (96, 128))], ids=["1-scale-48x64", "3-scales-96x128"])
def test_uniform_pipeline_acquire_and_launch_have_the_bits_of_submit(nscales, size):
    """ImagePairPipeline both ways at B = 2, N = 24: three batches decoded into the pinned views of acquire() and launched -- the call
    sequence of bench.py -- equal submit() of the same arrays on a pipeline of its own.  Three scales run at 96 x 128: level 2 of a 48 x 64
    image (12 x 16) is smaller than a 16 x 16 patch, and extract_patches refuses such a batch whole."""
    from vtamiq_amd.pipeline import ImagePairPipeline
    m = _model(nscales)
    B, N = 2, 24
    rs = np.random.RandomState(23)
    a, b = ImagePairPipeline(m, B, size, N, num_scales=nscales), ImagePairPipeline(m, B, size, N, num_scales=nscales)
    got, want = [], []
    for it in range(3):
        items = [_image_and_samples(rs, size, N, nscales) for _ in range(2 * B)]
        img, smp, sid = (np.stack(_col(items, k)) for k in range(3))
        hi, hs, hd = a.acquire()
        assert hi.shape == img.shape and hs.shape == smp.shape and (hd is None) == (nscales == 1)
        hi[:], hs[:] = img, smp
        if hd is not None:
            hd[:] = sid
        got.append(a.launch())
        want.append(b.submit(img[:B], img[B:], smp, sid if nscales > 1 else None))
    torch.cuda.synchronize()
    assert a.count == b.count == 3
    for g, w in zip(got, want):
        assert g.shape == (B,) and same(g, w)
    assert not torch.equal(got[0], got[1])
    with torch.no_grad():
        pa, po, sc = extract_patches(torch.from_numpy(img).to(DEV), torch.from_numpy(smp).to(DEV),
                                     torch.from_numpy(sid).to(DEV) if nscales > 1 else None, nscales)
        direct = m((pa[:B], pa[B:]), (po[:B], po[B:]), (sc[:B], sc[B:]) if sc is not None else (None, None))[0]
    torch.cuda.synchronize()
    assert same(got[2], direct)
