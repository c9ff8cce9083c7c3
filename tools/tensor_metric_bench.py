"""Scoring image tensors that are already on the GPU: what the planar gather and ImageMetric cost (profiles/r20_tensor_metric.txt).

    VTQ_ALLOW_ABI_MISMATCH=1 python tools/tensor_metric_bench.py --parent-lib PATH [--out profiles/r20_tensor_metric.txt]
                                                                 [--steps 20] [--gather-steps 1000] [--warmup 5] [--reps 5] [--gathers-only]

ViT-B/16, L = 12, precision fp16x3 (explicit: no error-word read per call).  B = 32 pairs of 384 x 512 images, N = 500 patches each, one
scale and three.  HIP events around `steps` back-to-back calls after `warmup` calls, `reps` repetitions with the variants interleaved inside
each repetition; medians and min-to-max spread.  A gather takes tens of microseconds, so its window is `gather-steps` calls: the figure
is the time per call of a back-to-back stream of launches, which the kernel bounds only if it is longer than an enqueue -- for the kernels'
own times run the gathers alone under a kernel trace (`rocprofv3 --kernel-trace --stats -- python tools/tensor_metric_bench.py
--gathers-only ...`) and read the per-kernel averages.  --parent-lib: a build of the parent commit's library (it lacks this commit's entry, so it
loads with VTQ_ALLOW_ABI_MISMATCH=1 beside it); without it the [parent] variants run on this library and say so.
  (a) the gathers alone, on the same device-sampled coordinates of the 64 images:
      u8 [parent]             vtq_k_gather_patches_u8 of the parent's library on the uint8 HWC images
      planar fp32|fp16|bf16   vtq_k_gather_patches_planar on the same pixels as float CHW planes
      each as a time and as image bytes read per second (from the code: a level-s patch reads 3 (P 2^s)^2 elements).  The float kernels read
      4 x / 2 x the bytes of the u8 one and have no table; the file says whether each is within that ratio of the u8 time.  No gate.
  (b) ImageMetric per batch on resident fp32 tensors against forward_varlen on resident patches of the same lengths: the difference is
      the sampler plus the two gathers plus the host's planning.
  (c) the unchanged paths, this library against the parent's in the same interleaved run: forward() on resident patches and
      ImagePairVarlenPipeline.submit_images on host uint8 images (front end and engine both on the library named)."""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, ImageMetric, _lib, synth  # noqa: E402
from vtamiq_amd.patches import extract_patches_planar, gather_patches_planar, image_tables  # noqa: E402
from vtamiq_amd.pipeline import ImagePairVarlenPipeline  # noqa: E402
from vtamiq_amd.sampling import sample_patches  # noqa: E402

DEV = "cuda"
(H, W), B, N, P = (384, 512), 32, 500, 16
HALF = (0.5, 0.5, 0.5)


class ParentVTAMIQ(VTAMIQ):
    """The same model on another build of the engine library."""
    LIB = None

    def _engine_lib(self):
        return _lib.load(self.LIB)


@contextlib.contextmanager
def library(path):
    """Everything that asks for the product library inside the block (gather, sampler, reductions) gets `path`."""
    keep, _lib.LIB_PATH = _lib.LIB_PATH, path or _lib.LIB_PATH
    try:
        yield
    finally:
        _lib.LIB_PATH = keep


def make_model(nscales=1, cls=VTAMIQ):
    m = cls(vit_config=dict(variant="ViT-B16", num_scales=nscales if nscales > 1 else 0, pretrained=False), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 0).items()})
    return m.to(DEV).eval()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))


def gather_case(nscales, parent_lib, images_u8):
    """(variants, element counts read per call): the five gathers on one set of coordinates."""
    NI = images_u8.shape[0]
    sizes = [(H, W)] * NI
    smp, sid, lengths = sample_patches(sizes, N, list(range(NI)), seed=1, num_scales=nscales, device=DEV)
    levels = np.bincount(sid.cpu().numpy() if sid is not None else np.zeros(NI * N, np.int64), minlength=nscales)
    elements = int(sum(int(n) * 3 * (P << s) ** 2 for s, n in enumerate(levels)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t8 = image_tables(sizes, lengths)
    tab8, pimg = dev(t8.tab), dev(t8.patch_img)
    flat8 = images_u8.reshape(-1)
    out = [torch.empty(t8.total, 3, P, P, device=DEV), torch.empty(t8.total, 2, device=DEV), torch.empty(t8.total, device=DEV)]
    f3 = (C.c_float * 3)(*HALF)
    as_p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib = _lib.load(parent_lib)

    def u8_parent():
        rc = lib.vtq_k_gather_patches_u8(flat8.data_ptr(), flat8.numel(), tab8.data_ptr(), pimg.data_ptr(), as_p(t8.img_off, C.c_int64),
                                         as_p(t8.H, C.c_int32), as_p(t8.W, C.c_int32), as_p(t8.row0, C.c_int32), NI, smp.data_ptr(),
                                         sid.data_ptr() if sid is not None else None, None, f3, f3, out[0].data_ptr(), out[1].data_ptr(),
                                         out[2].data_ptr() if sid is not None else None, P, nscales, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.vtq_last_error()
        return out[0]

    tag = f"{nscales}s"
    variants = {f"u8 [parent] {tag}": u8_parent}
    chw = images_u8.permute(0, 3, 1, 2).float().div(255)             # the same pixels as floats in CHW order
    want = u8_parent().clone()
    for name, dt in (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16)):
        flat = chw.to(dt).contiguous().reshape(-1)
        t = image_tables(sizes, lengths, flat.element_size())
        tab = dev(t.tab)
        variants[f"planar {name} {tag}"] = (lambda flat=flat, t=t, tab=tab:
                                            gather_patches_planar(flat, t, tab, pimg, smp, sid, None, nscales, HALF, HALF, P)[0])
    got = variants[f"planar fp32 {tag}"]()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) < 1e-5, "the planar gather disagrees with the u8 gather"
    return variants, elements, levels.tolist()


def metric_case(model, nscales, images_u8):
    ref = images_u8[:B].permute(0, 3, 1, 2).float().div(255).contiguous()
    dist = images_u8[B:].permute(0, 3, 1, 2).float().div(255).contiguous()
    metric = ImageMetric(model, patch_count=N, num_scales=nscales)
    smp, sid, lengths = sample_patches([(H, W)] * (2 * B), N, list(range(B)) * 2, seed=0, num_scales=nscales, device=DEV)
    pa, po, sc = extract_patches_planar(torch.cat([ref, dist]), smp, lengths, sid, nscales, validate=False)
    T = B * N
    scs = (sc[:T], sc[T:]) if sc is not None else (None, None)
    tag = f"{nscales}s"
    variants = {f"ImageMetric fp32 {tag}": lambda: metric(ref, dist),
                f"forward_varlen resident {tag}": lambda: model.forward_varlen((pa[:T], pa[T:]), (po[:T], po[T:]), scs, [N] * B)[0]}
    q = ImageMetric(model, patch_count=N, num_scales=nscales)(ref, dist, keys=list(range(B)))
    torch.cuda.synchronize()
    assert torch.equal(q, variants[f"forward_varlen resident {tag}"]()), "ImageMetric disagrees with forward_varlen on its patches"
    return variants


def unchanged_case(model, parent_model, parent_lib, images_u8):
    rs = np.random.RandomState(2)
    spec = model.spec
    p, pos, _ = synth.make_inputs(spec, B, N, 3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = ((dev(p[:, 0]), dev(p[:, 1])), (dev(pos[:, 0]), dev(pos[:, 1])), (None, None))
    host = images_u8.cpu().numpy()
    refs, dists = list(host[:B]), list(host[B:])
    cap = dict(max_pairs=B, max_image_bytes=2 * B * 3 * H * W, max_patches=B * N)
    pipe = ImagePairVarlenPipeline(model, **cap)
    with library(parent_lib):
        parent_pipe = ImagePairVarlenPipeline(parent_model, **cap)
    keys = [int(k) for k in rs.randint(0, 2 ** 31, size=B)]

    def parent_submit():
        with library(parent_lib):
            return parent_pipe.submit_images(refs, dists, N, keys=keys)

    variants = {"forward": lambda: model(*args)[0], "forward [parent]": lambda: parent_model(*args)[0],
                "submit_images": lambda: pipe.submit_images(refs, dists, N, keys=keys), "submit_images [parent]": parent_submit}
    q = {k: f() for k, f in variants.items()}
    torch.cuda.synchronize()
    same = torch.equal(q["forward"], q["forward [parent]"]) and torch.equal(q["submit_images"], q["submit_images [parent]"])
    return variants, same


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r20_tensor_metric.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--gather-steps", type=int, default=1000)
    ap.add_argument("--gathers-only", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/tensor_metric_bench.py measures on the GPU: no device found")
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None
    rs = np.random.RandomState(0)
    images_u8 = torch.from_numpy(rs.randint(0, 256, size=(2 * B, H, W, 3), dtype=np.uint8)).to(DEV)
    with torch.no_grad():
        m1, m3 = make_model(1), make_model(3)
        ParentVTAMIQ.LIB = parent_lib
        parent = make_model(1, ParentVTAMIQ)
        g1, e1, l1 = gather_case(1, parent_lib, images_u8)
        g3, e3, l3 = gather_case(3, parent_lib, images_u8)
        groups = [("(a) gathers alone, one scale", g1), ("(a) gathers alone, three scales", g3)]
        if a.gathers_only:                                            # for a kernel trace: a few calls of each, nothing written
            for _, variants in groups:
                for fn in variants.values():
                    timed(fn, a.steps, a.warmup)
            return
        un, same_bits = unchanged_case(m1, parent, parent_lib, images_u8)
        groups += [("(b) ImageMetric, one scale", metric_case(m1, 1, images_u8)), ("(b) ImageMetric, three scales", metric_case(m3, 3, images_u8)),
                   ("(c) unchanged paths", un)]
        times = {k: [] for _, v in groups for k in v}
        for _ in range(a.reps):
            for title, variants in groups:
                for k, fn in variants.items():
                    times[k].append(timed(fn, a.gather_steps if title.startswith("(a)") else a.steps, a.warmup))
    st = {k: stats(v) for k, v in times.items()}
    med = {k: s["median"] for k, s in st.items()}
    lines = [f"tools/tensor_metric_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit)",
             f"ms per call, {a.reps} repetitions of {a.steps} steps ((a): {a.gather_steps}) behind {a.warmup} warm-ups (HIP events), variants interleaved; "
             f"[parent] = the parent commit's library ({'given' if parent_lib else 'NOT given: this library stands in for it'})",
             f"B = {B} pairs of {H} x {W}, N = {N} patches per image, P = {P}; patches per level of the 64 images: one scale {l1}, three scales {l3}"]
    for title, variants in groups:
        lines += ["", title, f"{'variant':<32}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
        for k in variants:
            s = st[k]
            lines.append(f"{k:<32}{s['median']:>10.4f}{s['min']:>10.4f}{s['max']:>10.4f}{s['spread']:>10.4f}   " + " ".join(f"{t:.4f}" for t in times[k]))
    lines.append("")
    verdicts = {}
    for ns, elements in ((1, e1), (3, e3)):
        u = med[f"u8 [parent] {ns}s"]
        lines.append(f"(a) {ns} scale(s): {elements / 1e6:.1f} M pixel elements read per call; u8 [parent] {u:.4f} ms = {elements / u / 1e6:.1f} GB/s of image bytes")
        for name, elem in (("fp32", 4), ("fp16", 2), ("bf16", 2)):
            t = med[f"planar {name} {ns}s"]
            ok = t <= elem * u
            verdicts[f"{name} {ns}s"] = dict(ratio=t / u, byte_ratio=elem, within=ok)
            lines.append(f"    planar {name}: {t:.4f} ms = {elements * elem / t / 1e6:.1f} GB/s; {t / u:.2f} x the u8 time for {elem} x the bytes: "
                         + ("within its byte ratio" if ok else "NOT within its byte ratio"))
    if not all(v["within"] for v in verdicts.values()):
        lines.append("    where a float kernel is not within its byte ratio: it normalises every level-0 pixel it pools in registers -- a subtraction and a "
                     "true division each, 4^s per output element and channel -- where the u8 kernel looks a byte up in a 3 x 256 table; its cost per "
                     "element does not shrink with the element size")
    for ns in (1, 3):
        im, fv = med[f"ImageMetric fp32 {ns}s"], med[f"forward_varlen resident {ns}s"]
        lines.append(f"(b) {ns} scale(s): ImageMetric {im:.3f} ms per batch, forward_varlen on resident patches {fv:.3f} ms: sampler + two gathers + "
                     f"planning = {im - fv:.3f} ms ({fv / im:.3f} of the call is the forward)")
    for k in ("forward", "submit_images"):
        d = med[k] - med[k + " [parent]"]
        spread = max(st[k]["spread"], st[k + " [parent]"]["spread"])
        lines.append(f"(c) {k}: {med[k]:.3f} ms against {med[k + ' [parent]']:.3f} ms on the parent's library: {d:+.3f} ms, the run's own spread is "
                     f"{spread:.3f} ms: " + ("within it" if abs(d) <= spread else "OUTSIDE it"))
    lines += [f"(c) forward and submit_images bit-identical between the two libraries: {same_bits}", "",
              "json: " + json.dumps(dict(times=st, gathers=verdicts, elements=dict(one=e1, three=e3)))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
