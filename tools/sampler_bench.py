"""Sampling patch coordinates on the device against sampling them on the submitting thread (profiles/r16_sampler.txt).

    python tools/sampler_bench.py [--out profiles/r16_sampler.txt] [--steps 20] [--warmup 5] [--reps 5] [--parent-lib PATH]

ViT-B/16, L = 12, precision fp16x3 (explicit), the batches of tools/image_varlen_bench.py: 32 pairs, 8 each of 288 x 288, 384 x 512,
512 x 512 and 480 x 720 with patch counts proportional to the area around 500, and the uniform batch of 32 pairs of 384 x 512, N = 500.
HIP events around `steps` back-to-back calls after `warmup` calls, `reps` repetitions with the variants interleaved inside each repetition;
medians.  Per batch:
  (a)  submit            ImagePairVarlenPipeline.submit with coordinates made ahead of the loop -- measured THREE times per repetition
                         (a, a', a''), each on a pipeline of its own: the min-to-max distance of the three medians is the spread the
                         condition below allows
  (b)  submit + numpy    submit with the numpy restatement of the sampler (tests/sampler_model.py) run on the submitting thread inside
                         the loop: what a user without the device sampler does (the reference's Python is not part of this repository)
  (c)  submit_images     coordinates sampled on the device
  (d)  sampler alone     vtq_k_sample_grid on resident tables
  (a)  [parent]          (a) with the model on the parent commit's library (--parent-lib), to show it unchanged
Condition: (c) is no slower than (a) -- the middle one of its three medians -- by more than the spread of those three medians.
(b) / (c) is recorded as the gain, whatever it is."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from image_varlen_bench import PER_SIZE, RAGGED, UB, UN, UNIFORM, ParentVTAMIQ, make_model, stats, timed  # noqa: E402
from tests import sampler_model as SM  # noqa: E402
from vtamiq_amd import sampling  # noqa: E402
from vtamiq_amd.pipeline import ImagePairVarlenPipeline  # noqa: E402

DEV = "cuda"
SEED = 16


def case(model, parent_model, sizes, counts):
    rs = np.random.RandomState(0)
    B = len(sizes)
    refs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    dists = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    keys = list(range(B))
    cap = dict(max_pairs=B, max_image_bytes=2 * sum(3 * h * w for h, w in sizes), max_patches=sum(counts))
    pipes = {k: ImagePairVarlenPipeline(model, **cap) for k in ("a", "a'", "a''", "b", "c")}
    ahead = SM.per_image(sizes, counts, keys, SEED)[0]
    plan = sampling.plan_samples(sizes, counts)
    seg, seg_keys = np.ascontiguousarray(plan.seg), np.ascontiguousarray(np.asarray(keys, np.uint64)[plan.seg_image])
    dseg, dkeys = torch.from_numpy(seg).to(DEV), torch.from_numpy(seg_keys.view(np.int64)).to(DEV)
    out = torch.empty(plan.total, 2, dtype=torch.int32, device=DEV)
    variants = {
        "(a)  submit": lambda: pipes["a"].submit(refs, dists, ahead),
        "(b)  submit + numpy sampler": lambda: pipes["b"].submit(refs, dists, SM.per_image(sizes, counts, keys, SEED)[0]),
        "(c)  submit_images": lambda: pipes["c"].submit_images(refs, dists, counts, keys=keys, seed=SEED),
        "(a') submit": lambda: pipes["a'"].submit(refs, dists, ahead),
        "(a'') submit": lambda: pipes["a''"].submit(refs, dists, ahead),
        "(d)  sampler alone": lambda: sampling.launch_sample_grid(dseg, dkeys, seg, seg_keys, SEED, 13107, out, None),
    }
    if parent_model is not None:
        pp = ImagePairVarlenPipeline(parent_model, **cap)
        variants["(a)  submit [parent]"] = lambda: pp.submit(refs, dists, ahead)
    q = {k: f() for k, f in variants.items() if not k.startswith("(d)")}
    variants["(d)  sampler alone"]()
    torch.cuda.synchronize()
    first = q["(a)  submit"]
    assert all(torch.equal(x, first) for x in q.values()) and bool(torch.isfinite(first).all()), "the variants disagree"
    assert np.array_equal(out.cpu().numpy(), np.concatenate(ahead)), "the device samples are not the restatement's"
    return variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_sampler.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/sampler_bench.py measures on the GPU: no device found")
    with torch.no_grad():
        model, parent = make_model(1), None
        if a.parent_lib:
            ParentVTAMIQ.LIB = a.parent_lib
            parent = make_model(1, ParentVTAMIQ)
        mean_area = sum(h * w for h, w in RAGGED) / len(RAGGED)
        rcounts = [int(round(500 * h * w / mean_area)) for h, w in RAGGED]
        groups = [("ragged: 32 pairs, 8 each of " + ", ".join(f"{h} x {w}" for h, w in RAGGED) + f" with {rcounts} patches",
                   case(model, parent, [s for s in RAGGED for _ in range(PER_SIZE)], [n for n in rcounts for _ in range(PER_SIZE)])),
                  (f"uniform: {UB} pairs of {UNIFORM[0]} x {UNIFORM[1]}, N = {UN}", case(model, parent, [UNIFORM] * UB, [UN] * UB))]
        times = [{k: [] for k in v} for _, v in groups]
        for _ in range(a.reps):
            for t, (_, variants) in zip(times, groups):
                for k, fn in variants.items():
                    t[k].append(timed(fn, a.steps, a.warmup))
    lines = [f"tools/sampler_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit)",
             f"ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved; "
             f"[parent] = the model on the parent commit's library ({'given' if a.parent_lib else 'NOT given'})"]
    summary = {}
    for (title, variants), t in zip(groups, times):
        st = {k: stats(v) for k, v in t.items()}
        lines += ["", title, f"{'variant':<32}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
        for k in variants:
            s = st[k]
            lines.append(f"{k:<32}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{x:.3f}" for x in t[k]))
        b, c = st["(b)  submit + numpy sampler"]["median"], st["(c)  submit_images"]["median"]
        meds = sorted(st[k]["median"] for k in ("(a)  submit", "(a') submit", "(a'') submit"))
        a1, allowed = meds[1], meds[2] - meds[0]
        ok = c - a1 <= allowed
        lines += [f"medians of (a), (a'), (a''): {meds[0]:.3f} {meds[1]:.3f} {meds[2]:.3f} ms; (c) - (a) = {c - a1:+.3f} ms against their spread of "
                  f"{allowed:.3f} ms -> condition {'MET' if ok else 'NOT MET'}",
                  f"(c) / (a) = {c / a1:.4f};  gain (b) / (c) = {b / c:.3f};  sampler alone (d) = {1e3 * st['(d)  sampler alone']['median']:.1f} us"]
        if parent is not None:
            lines.append(f"(a) / (a) [parent] = {a1 / st['(a)  submit [parent]']['median']:.4f}")
        summary[title.split(":")[0]] = dict(times=st, condition_met=bool(ok))
    lines += ["scores bit-identical between (a), (b), (c) and [parent]; device samples equal to the restatement's: True", "",
              "json: " + json.dumps(summary)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
