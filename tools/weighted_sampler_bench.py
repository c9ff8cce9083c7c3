"""What placing patches where a pair differs costs on the device (profiles/r17_weighted_sampler.txt).

    python tools/weighted_sampler_bench.py [--out profiles/r17_weighted_sampler.txt] [--steps 20] [--warmup 5] [--reps 5]
    python tools/weighted_sampler_bench.py --host-only --reference /path/to/the/reference/checkout [--out ...]     (no GPU needed; appends)

ViT-B/16, L = 12, precision fp16x3 (explicit), the two batches of tools/sampler_bench.py: 32 pairs, 8 each of 288 x 288, 384 x 512,
512 x 512 and 480 x 720 with patch counts proportional to the area around 500, and the uniform batch of 32 pairs of 384 x 512, N = 500.
The distorted image of a pair is its reference with one region (1 / 16 of the image) replaced.  HIP events around `steps` back-to-back
calls after `warmup` calls, `reps` repetitions with the variants interleaved inside each repetition; medians.  Per batch:
  (a)  submit                    ImagePairVarlenPipeline.submit with coordinates made ahead of the loop, THREE times per repetition (a, a',
                                 a''), each on a pipeline of its own: the min-to-max distance of the three medians is submit()'s own spread
  (c)  submit_images             the default sampler (uniform SIMPLE grid) on the device
  (w)  submit_images weighted    sampler=WeightedPatchSampler(1.0, 0.1): difference pass + weighted sampler on the copy stream
  (p)  difference pass alone     vtq_k_diff_cells on resident images and tables; its bytes (2 images of 3 H W per pair) over its time
  (m)  device-to-device copy     of the same number of bytes, timed in the same run
  (s)  weighted sampler alone    vtq_k_sample_weighted on the resident table of (p), both images of every pair
  (r4) num_repeats = 4           one weighted submission with four samplings per pair, against
  (4x) four submissions          four weighted submissions of the batch
and, once, the sampler alone on one segment of 8100 samples, all in one cell and spread over sixteen.
The report says whether (w) - (a) stays inside the spread of (a)'s three medians, and where the time goes when it does not.
--host-only measures the reference's own Python (compute_diff and the weighted stratified_grid_sampling, one core) on the machine it runs
on and appends the figures to the profile, stated as such."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
SEED = 17
DW, UW = 1.0, 0.1


def make_pairs(sizes):
    rs = np.random.RandomState(0)
    refs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    dists = []
    for r in refs:
        d = r.copy()
        h, w = d.shape[:2]
        d[h // 2: 3 * h // 4, w // 4: w // 2] = rs.randint(0, 256, size=(3 * h // 4 - h // 2, w // 2 - w // 4, 3), dtype=np.uint8)
        dists.append(d)
    return refs, dists


def case(model, sizes, counts):
    from tests import sampler_model as SM
    from vtamiq_amd import sampling
    from vtamiq_amd.pipeline import ImagePairVarlenPipeline
    B = len(sizes)
    refs, dists = make_pairs(sizes)
    keys = list(range(B))
    nbytes = 2 * sum(3 * h * w for h, w in sizes)
    cap = dict(max_pairs=B, max_image_bytes=nbytes, max_patches=sum(counts))
    pipes = {k: ImagePairVarlenPipeline(model, **cap) for k in ("a", "a'", "a''", "c", "w", "4x")}
    pipes["r4"] = ImagePairVarlenPipeline(model, max_pairs=4 * B, max_image_bytes=nbytes, max_patches=4 * sum(counts))
    ahead = SM.per_image(sizes, counts, keys, SEED)[0]
    ws = sampling.WeightedPatchSampler(DW, UW)
    # resident images and tables for the kernels alone
    flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in refs + dists])).to(DEV)
    off = np.concatenate([[0], np.cumsum([im.size for im in refs + dists])[:-1]])
    plan = sampling.plan_samples_weighted(list(sizes) * 2, list(counts) * 2, pair_of=list(range(B)) * 2)
    pairs = plan.pairs.copy()
    pairs[:, 0], pairs[:, 1] = off[:B], off[B:]
    seg, lev = np.ascontiguousarray(plan.seg), np.ascontiguousarray(plan.lev)
    seg_keys = np.ascontiguousarray(np.asarray(keys * 2, np.uint64)[plan.seg_image])
    dpairs, dlev, dseg = torch.from_numpy(pairs).to(DEV), torch.from_numpy(lev).to(DEV), torch.from_numpy(seg).to(DEV)
    dkeys = torch.from_numpy(seg_keys.view(np.int64)).to(DEV)
    tab = torch.empty(plan.tab_words, dtype=torch.int64, device=DEV)
    out = torch.empty(plan.total, 2, dtype=torch.int32, device=DEV)
    twin = torch.empty_like(flat)

    def four():
        for _ in range(4):
            q = pipes["4x"].submit_images(refs, dists, counts, keys=keys, seed=SEED, sampler=ws)
        return q

    variants = {
        "(a)  submit": lambda: pipes["a"].submit(refs, dists, ahead),
        "(c)  submit_images": lambda: pipes["c"].submit_images(refs, dists, counts, keys=keys, seed=SEED),
        "(w)  submit_images weighted": lambda: pipes["w"].submit_images(refs, dists, counts, keys=keys, seed=SEED, sampler=ws),
        "(a') submit": lambda: pipes["a'"].submit(refs, dists, ahead),
        "(p)  difference pass alone": lambda: sampling.launch_diff_cells(flat, dpairs, dlev, pairs, lev, 16, tab, plan.tab_words),
        "(m)  device-to-device copy": lambda: twin.copy_(flat),
        "(s)  weighted sampler alone": lambda: sampling.launch_sample_weighted(dseg, dkeys, seg, seg_keys, 16, tab, plan.tab_words, ws, SEED, out, None),
        "(a'') submit": lambda: pipes["a''"].submit(refs, dists, ahead),
        "(r4) num_repeats = 4": lambda: pipes["r4"].submit_images(refs, dists, counts, keys=keys, seed=SEED, num_repeats=4, sampler=ws),
        "(4x) four submissions": four,
    }
    q = {k: f() for k, f in variants.items()}
    torch.cuda.synchronize()
    assert torch.equal(q["(a)  submit"], q["(c)  submit_images"]) and torch.equal(q["(a)  submit"], q["(a') submit"]), "the default paths disagree"
    qw = q["(w)  submit_images weighted"]
    assert bool(torch.isfinite(qw).all()) and not torch.equal(qw, q["(a)  submit"]) and torch.equal(qw, q["(4x) four submissions"])
    smp = out.cpu().numpy().astype(np.int64)
    n0 = int(seg[0, 1])                                              # the first reference's level-0 rows: how many touch the region that differs
    h, w = sizes[0]
    s0 = smp[:n0]
    share = float(((s0[:, 0] + 16 > h // 2) & (s0[:, 0] < 3 * h // 4) & (s0[:, 1] + 16 > w // 4) & (s0[:, 1] < w // 2)).mean())
    return variants, nbytes, share


def big_cell_case():
    """The sampler alone on ONE segment at the limit of 8100 samples on a 64 x 64 level (16 cells): every sample in one cell (wd = 90,
    8100 sub-cells ranked by the whole workgroup), and the same count spread uniformly."""
    from tests import weighted_sampler_model as WM
    from vtamiq_amd import sampling
    n, P = 8100, 16
    cs, sh, sw = sampling.cell_geometry(n, 64, 64, P)
    m = np.zeros((64, 64), np.int64)
    m[:5, :5] = 100
    tab = torch.from_numpy(WM.map_table(m, cs, sh, sw, P).view(np.int64)).to(DEV)
    seg = np.asarray([[0, n, cs, sh, sw, 64 - P, 64 - P, 0, 0, 4, 0, 0]], np.int32)
    keys = np.asarray([5], np.uint64)
    dseg, dkeys = torch.from_numpy(seg).to(DEV), torch.from_numpy(keys.view(np.int64)).to(DEV)
    out = torch.empty(n, 2, dtype=torch.int32, device=DEV)
    one, spread = sampling.WeightedPatchSampler(1.0, 0.0), sampling.WeightedPatchSampler(1.0, 1e6)
    fn = lambda ws: (lambda: sampling.launch_sample_weighted(dseg, dkeys, seg, keys, P, tab, tab.numel(), ws, SEED, out, None))
    fn(one)()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), WM.segment(SEED, 5, 0, n, cs, sh, sw, 64 - P, 64 - P, P, 13107, 1.0, 0.0, WM.map_table(m, cs, sh, sw, P), 0, 4).samples)
    return {"(s1)  8100 samples in one cell": fn(one), "(s16) 8100 samples over 16 cells": fn(spread)}


def host_cost(reference, out):
    """The reference's own Python on this machine's CPU, one core: compute_diff on a 384 x 512 pair and weighted sampling at n = 500."""
    sys.path.insert(0, os.path.abspath(reference))

    def view_as_windows(arr, shape, step):
        return np.lib.stride_tricks.sliding_window_view(arr, shape)[::step[0], ::step[1]]

    try:
        import skimage.util.shape  # noqa: F401
    except ImportError:
        for name in ("skimage", "skimage.util", "skimage.util.shape"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["skimage.util.shape"].view_as_windows = view_as_windows
    torch.set_num_threads(1)
    from data import patch_sampling as R
    if getattr(R, "view_as_windows", None) is None:
        R.view_as_windows = view_as_windows
    refs, dists = make_pairs([(384, 512)])
    s = R.PatchSampler(diff_weight=DW, uniform_weight=UW, grid_type=R.GRID_TYPE_PERTURBED)
    np.random.seed(0)

    def ms(fn, n):
        fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(t)), min(t), max(t)

    diff = s.compute_diff([refs[0], dists[0]])
    d = ms(lambda: s.compute_diff([refs[0], dists[0]]), 20)
    g = ms(lambda: s(384, 512, 16, 16, diff=diff, num_samples=500), 20)
    lines = ["", "the reference's host cost per pair, measured on a CPU-only machine (one core, the reference's own Python; not the GPU machine above):",
             f"compute_diff on a 384 x 512 pair: median {d[0]:.2f} ms (min {d[1]:.2f}, max {d[2]:.2f}) of 20 calls",
             f"weighted stratified_grid_sampling, n = 500: median {g[0]:.2f} ms (min {g[1]:.2f}, max {g[2]:.2f}) of 20 calls",
             f"together {d[0] + g[0]:.1f} ms per pair"]
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_weighted_sampler.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    if a.host_only:
        if not a.reference:
            sys.exit("--host-only needs --reference")
        return host_cost(a.reference, a.out)
    if not torch.cuda.is_available():
        sys.exit("tools/weighted_sampler_bench.py measures on the GPU: no device found")
    from image_varlen_bench import PER_SIZE, RAGGED, UB, UN, UNIFORM, make_model, stats, timed
    with torch.no_grad():
        model = make_model(1)
        mean_area = sum(h * w for h, w in RAGGED) / len(RAGGED)
        rcounts = [int(round(500 * h * w / mean_area)) for h, w in RAGGED]
        groups = [("ragged: 32 pairs, 8 each of " + ", ".join(f"{h} x {w}" for h, w in RAGGED) + f" with {rcounts} patches",
                   case(model, [s for s in RAGGED for _ in range(PER_SIZE)], [n for n in rcounts for _ in range(PER_SIZE)])),
                  (f"uniform: {UB} pairs of {UNIFORM[0]} x {UNIFORM[1]}, N = {UN}", case(model, [UNIFORM] * UB, [UN] * UB))]
        times = [{k: [] for k in v[0]} for _, v in groups]
        big = big_cell_case()
        big_times = {k: [] for k in big}
        for _ in range(a.reps):
            for t, (_, (variants, _, _)) in zip(times, groups):
                for k, fn in variants.items():
                    t[k].append(timed(fn, a.steps, a.warmup))
            for k, fn in big.items():
                big_times[k].append(timed(fn, a.steps, a.warmup))
    lines = [f"tools/weighted_sampler_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit), "
             f"WeightedPatchSampler({DW}, {UW})",
             f"ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved"]
    summary = {}
    for (title, (variants, nbytes, share)), t in zip(groups, times):
        st = {k: stats(v) for k, v in t.items()}
        lines += ["", title, f"{'variant':<32}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
        for k in variants:
            s = st[k]
            lines.append(f"{k:<32}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{x:.3f}" for x in t[k]))
        med = lambda k: st[k]["median"]
        meds = sorted(med(k) for k in ("(a)  submit", "(a') submit", "(a'') submit"))
        a1, allowed = meds[1], meds[2] - meds[0]
        w, c, p, m, s_ = med("(w)  submit_images weighted"), med("(c)  submit_images"), med("(p)  difference pass alone"), med("(m)  device-to-device copy"), med("(s)  weighted sampler alone")
        inside = w - a1 <= allowed
        lines += [f"medians of (a), (a'), (a''): {meds[0]:.3f} {meds[1]:.3f} {meds[2]:.3f} ms; (w) - (a) = {w - a1:+.3f} ms, (c) - (a) = {c - a1:+.3f} ms, against "
                  f"their spread of {allowed:.3f} ms -> the weighted sampler's added time is {'INSIDE' if inside else 'OUTSIDE'} submit()'s own spread",
                  f"difference pass alone: {1e3 * p:.1f} us for {nbytes / 1e6:.1f} MB = {nbytes / p / 1e6:.0f} GB/s read; a device-to-device copy of the same "
                  f"bytes: {1e3 * m:.1f} us = {nbytes / m / 1e6:.0f} GB/s read (and as much written); weighted sampler alone: {1e3 * s_:.1f} us",
                  f"the kernels alone, (p) + (s) = {p + s_:.3f} ms, are {100 * (p + s_) / a1:.1f} % of (a); (w) - (c) = {w - c:+.3f} ms.  They run on the "
                  "copy stream beside the previous batch's forward, which fills the chip: the time they take there is taken from that forward "
                  "(supposed from these figures, not traced)" + ("" if inside else
                                                                "; the difference pass, which reads at a fraction of the copy's rate, is where that time goes"),
                  f"num_repeats = 4: {med('(r4) num_repeats = 4'):.3f} ms against four submissions {med('(4x) four submissions'):.3f} ms = "
                  f"{med('(r4) num_repeats = 4') / med('(4x) four submissions'):.3f}",
                  f"level-0 patches of the first reference that touch the region that differs (1 / 16 of the image): {100 * share:.0f} %"]
        summary[title.split(":")[0]] = dict(times=st, inside_spread=bool(inside), diff_pass_GBps=nbytes / p / 1e6, copy_GBps=nbytes / m / 1e6)
    lines += ["", "the weighted sampler alone on one segment of 8100 samples (the limit) on a 64 x 64 level, ms per launch; the rows equal the restatement's",
              f"{'variant':<36}{'median':>10}{'min':>10}{'max':>10}"]
    for k, v in big_times.items():
        st = stats(v)
        lines.append(f"{k:<36}{st['median']:>10.3f}{st['min']:>10.3f}{st['max']:>10.3f}")
    lines += ["", "json: " + json.dumps(summary)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
