"""The image front end for images of different sizes against what a user did before it (profiles/r15_image_varlen.txt).

    python tools/image_varlen_bench.py [--out profiles/r15_image_varlen.txt] [--steps 20] [--warmup 5] [--reps 5] [--parent-lib PATH]

ViT-B/16, L = 12, precision fp16x3 (explicit: no error-word read per call).  HIP events around `steps` back-to-back calls after `warmup`
calls, `reps` repetitions with the variants interleaved inside each repetition; medians and min-to-max spread.
  (a) a ragged batch: 32 pairs, 8 each of 288 x 288, 384 x 512, 512 x 512 and 480 x 720, patch counts proportional to the area around 500
      ragged_pipeline       ImagePairVarlenPipeline.submit: host images in, one gather over the 64 images, forward_varlen
      four_pipelines        four ImagePairPipelines, one per size (8 pairs each): what a user did before; with --parent-lib the model runs on
                            THAT library (the front end's kernels are unchanged since the parent, so they come from this one)
      varlen_resident       forward_varlen alone on the same patches, resident on the device: the pipeline's efficiency is measured against it
  (b) uniform shapes, B = 32, 384 x 512, N = 500, one scale and three: what the fused gather itself costs
      gather_u8 / extract_patches   the front ends alone on resident uint8 images (kernel time: vtq_k_gather_patches_u8 against
                                    normalise + pyramid + gather)
      pipeline_varlen / pipeline    the two pipelines end to end
      varlen_resident / forward_resident   what they end in, forward_varlen at equal lengths and forward(), on resident patches
No ratio is a bar here; the numbers are recorded."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, _lib, synth  # noqa: E402
from vtamiq_amd.patches import extract_patches, gather_patches_u8, image_tables  # noqa: E402
from vtamiq_amd.pipeline import ImagePairPipeline, ImagePairVarlenPipeline  # noqa: E402

DEV = "cuda"
RAGGED = [(288, 288), (384, 512), (512, 512), (480, 720)]
PER_SIZE = 8
UNIFORM, UB, UN = (384, 512), 32, 500


class ParentVTAMIQ(VTAMIQ):
    """The same model on another build of the engine library."""
    LIB = None

    def _engine_lib(self):
        return _lib.load(self.LIB)


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


def sample(rs, h, w, n, nscales, P=16):
    sid = np.sort(rs.randint(0, nscales, size=n)).astype(np.int32)
    smp = np.stack([rs.randint(0, (h >> sid) - P + 1), rs.randint(0, (w >> sid) - P + 1)], axis=-1).astype(np.int32)
    return smp, sid


def ragged_case(model, parent_model):
    rs = np.random.RandomState(0)
    mean_area = sum(h * w for h, w in RAGGED) / len(RAGGED)
    counts = [int(round(500 * h * w / mean_area)) for h, w in RAGGED]
    sizes = [s for s in RAGGED for _ in range(PER_SIZE)]
    ns = [n for n in counts for _ in range(PER_SIZE)]
    refs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    dists = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    smp = [sample(rs, h, w, n, 1)[0] for (h, w), n in zip(sizes, ns)]
    nbytes = 2 * sum(3 * h * w for h, w in sizes)
    pipe = ImagePairVarlenPipeline(model, max_pairs=len(sizes), max_image_bytes=nbytes, max_patches=sum(ns))
    four = []
    for g, ((h, w), n) in enumerate(zip(RAGGED, counts)):
        k = slice(g * PER_SIZE, (g + 1) * PER_SIZE)
        four.append((ImagePairPipeline(parent_model or model, PER_SIZE, (h, w), n), np.stack(refs[k]), np.stack(dists[k]), np.stack(smp[k])))
    # the resident tensors of the same batch, through the new gather
    t = image_tables(sizes + sizes, ns + ns)
    flat = torch.from_numpy(np.concatenate([i.reshape(-1) for i in refs + dists])).to(DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pa, po, _ = gather_patches_u8(flat, t, dev(t.tab), dev(t.patch_img), dev(np.concatenate(smp + smp)), None, None, 1, (0.5,) * 3, (0.5,) * 3, 16)
    T = sum(ns)
    variants = {
        "ragged_pipeline": lambda: pipe.submit(refs, dists, smp),
        "four_pipelines" + (" [parent]" if parent_model else ""): lambda: torch.cat([p.submit(r, d, s) for p, r, d, s in four]),
        "varlen_resident": lambda: model.forward_varlen((pa[:T], pa[T:]), (po[:T], po[T:]), (None, None), ns)[0],
    }
    q = {k: f() for k, f in variants.items()}
    torch.cuda.synchronize()
    assert all(torch.equal(x, q["ragged_pipeline"]) for x in q.values()) and bool(torch.isfinite(q["ragged_pipeline"]).all()), "the variants disagree"
    info = dict(counts=counts, patches_per_side=T, image_bytes=nbytes)
    return variants, info


def uniform_case(model, nscales):
    rs = np.random.RandomState(1)
    (h, w), B, N = UNIFORM, UB, UN
    refs, dists = rs.randint(0, 256, size=(B, h, w, 3), dtype=np.uint8), rs.randint(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    ss = [sample(rs, h, w, N, nscales) for _ in range(B)]
    smp, sid = np.stack([s[0] for s in ss]), np.stack([s[1] for s in ss])
    old = ImagePairPipeline(model, B, (h, w), N, num_scales=nscales)
    new = ImagePairVarlenPipeline(model, max_pairs=B, max_image_bytes=2 * B * 3 * h * w, max_patches=B * N, num_scales=nscales)
    img = torch.from_numpy(np.concatenate([refs, dists])).to(DEV)
    s2, i2 = torch.from_numpy(np.concatenate([smp, smp])).to(DEV), (torch.from_numpy(np.concatenate([sid, sid])).to(DEV) if nscales > 1 else None)
    t = image_tables([(h, w)] * (2 * B), [N] * (2 * B))
    dtab, dpimg = torch.from_numpy(t.tab).to(DEV), torch.from_numpy(t.patch_img).to(DEV)
    flat, sf, jf = img.reshape(-1), s2.reshape(-1, 2), (i2.reshape(-1) if i2 is not None else None)
    lists = lambda a: [x for x in a]
    tag = f"{nscales}s"
    variants = {
        f"gather_u8 {tag}": lambda: gather_patches_u8(flat, t, dtab, dpimg, sf, jf, None, nscales, (0.5,) * 3, (0.5,) * 3, 16)[0],
        f"extract_patches {tag}": lambda: extract_patches(img, s2, i2, nscales, validate=False)[0],
        f"pipeline_varlen {tag}": lambda: new.submit(lists(refs), lists(dists), lists(smp), scale_ids=lists(sid) if nscales > 1 else None),
        f"pipeline {tag}": lambda: old.submit(refs, dists, smp, sid if nscales > 1 else None),
    }
    # what the two pipelines end in, on the same patches resident on the device: forward() and forward_varlen() at equal lengths
    pa, po, sc = extract_patches(img, s2, i2, nscales, validate=False)
    scs = (sc[:B], sc[B:]) if sc is not None else (None, None)
    flat2 = lambda x: x.reshape(-1, *x.shape[2:])
    scv = (flat2(sc[:B]), flat2(sc[B:])) if sc is not None else (None, None)
    variants[f"forward_resident {tag}"] = lambda: model((pa[:B], pa[B:]), (po[:B], po[B:]), scs)[0]
    variants[f"varlen_resident {tag}"] = lambda: model.forward_varlen((flat2(pa[:B]), flat2(pa[B:])), (flat2(po[:B]), flat2(po[B:])), scv, [N] * B)[0]
    a, b = variants[f"gather_u8 {tag}"](), variants[f"extract_patches {tag}"]()
    qa, qb = variants[f"pipeline_varlen {tag}"](), variants[f"pipeline {tag}"]()
    torch.cuda.synchronize()
    assert torch.equal(a.view(b.shape), b) and torch.equal(qa, qb) and bool(torch.isfinite(qa).all()), "the two front ends disagree"
    return variants


def bytes_moved(h, w, NI, N, nscales, P=16):
    """From the code, per call, in MB: what each front end reads + writes in device memory (cache hits not subtracted)."""
    px = NI * h * w
    pyr = sum(px // 4 ** s for s in range(1, nscales))
    out = NI * N * (3 * P * P + 2 + (1 if nscales > 1 else 0)) * 4
    old = 3 * px + 12 * px + sum(12 * (px // 4 ** (s - 1)) + 12 * (px // 4 ** s) for s in range(1, nscales)) + (out - 0) + NI * N * 3 * P * P * 4
    per_level = [NI * N // nscales * 3 * P * P * 4 ** s for s in range(nscales)]         # uint8 source bytes of a level-s patch, levels equally used
    new = sum(per_level) + out
    return dict(old_mb=old / 1e6, old_intermediate_mb=(12 * px + 12 * pyr) / 1e6, new_mb=new / 1e6, new_intermediate_mb=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15_image_varlen.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/image_varlen_bench.py measures on the GPU: no device found")
    parent = None
    with torch.no_grad():
        m1, m3 = make_model(1), make_model(3)
        if a.parent_lib:
            ParentVTAMIQ.LIB = a.parent_lib
            parent = make_model(1, ParentVTAMIQ)
        ragged, info = ragged_case(m1, parent)
        groups = [("(a) ragged batch", ragged), ("(b) uniform, one scale", uniform_case(m1, 1)), ("(b) uniform, three scales", uniform_case(m3, 3))]
        times = {k: [] for _, v in groups for k in v}
        for _ in range(a.reps):
            for _, variants in groups:
                for k, fn in variants.items():
                    times[k].append(timed(fn, a.steps, a.warmup))
    st = {k: stats(v) for k, v in times.items()}
    med = {k: s["median"] for k, s in st.items()}
    lines = [f"tools/image_varlen_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit)",
             f"ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved; "
             f"[parent] = the model on the parent commit's library ({'given' if a.parent_lib else 'NOT given: this library only'})",
             f"(a): 32 pairs, {PER_SIZE} each of {', '.join(f'{h} x {w}' for h, w in RAGGED)} with {info['counts']} patches "
             f"({info['patches_per_side']} per side, {info['image_bytes'] / 1e6:.1f} MB of uint8 images);  (b): B = {UB}, {UNIFORM[0]} x {UNIFORM[1]}, N = {UN}"]
    for title, variants in groups:
        lines += ["", title, f"{'variant':<28}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
        for k in variants:
            s = st[k]
            lines.append(f"{k:<28}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{t:.3f}" for t in times[k]))
    four = [k for k in med if k.startswith("four_pipelines")][0]
    lines += ["",
              f"(a) ragged_pipeline / {four} = {med['ragged_pipeline'] / med[four]:.3f}",
              f"(a) pipeline efficiency = varlen_resident / ragged_pipeline = {med['varlen_resident'] / med['ragged_pipeline']:.3f}   "
              "(the uniform pipeline's figure against forward(): 0.97 - 0.98)"]
    for ns in (1, 3):
        bm = bytes_moved(UNIFORM[0], UNIFORM[1], 2 * UB, UN, ns)
        g, e, pv, p = (med[f"{k} {ns}s"] for k in ("gather_u8", "extract_patches", "pipeline_varlen", "pipeline"))
        spread = max(st[f"gather_u8 {ns}s"]["spread"], st[f"extract_patches {ns}s"]["spread"])
        fr, vr = med[f"forward_resident {ns}s"], med[f"varlen_resident {ns}s"]
        lines += [f"(b) {ns} scale(s): efficiency pipeline / forward_resident = {fr / p:.3f}, pipeline_varlen / varlen_resident = {vr / pv:.3f};  "
                  f"forward_varlen / forward at equal lengths = {vr / fr:.3f}"]
        lines += [f"(b) {ns} scale(s): gather_u8 / extract_patches = {g / e:.3f} ({g:.3f} against {e:.3f} ms, spread {spread:.3f} ms);  "
                  f"pipeline_varlen / pipeline = {pv / p:.3f}",
                  f"    bytes per call from the code: old front end {bm['old_mb']:.1f} MB read + written, {bm['old_intermediate_mb']:.1f} MB of it image-sized "
                  f"fp32 intermediates it allocates; fused gather {bm['new_mb']:.1f} MB, no intermediate"]
    lines += ["scores and patches bit-identical between the front ends in every case: True", "",
              "json: " + json.dumps(dict(times=st, ragged=info))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
