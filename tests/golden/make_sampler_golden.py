"""Records how the reference's default patch sampler behaves -> tests/golden/sampler_reference.npz (recorded results only, a few KB).

    python tests/golden/make_sampler_golden.py --reference /path/to/the/reference/checkout

Runs the reference's PatchSampler() (GRID_TYPE_PERTURBED_SIMPLE, perturbed_amount 0.2) and its two count functions under fixed numpy seeds:
  per shape (h, w, n), K = 400 calls: how often each grid cell was chosen, the sums of the in-cell offsets, and the first eight calls raw;
  a table (H, W, patch_count, num_scales, ratio, P) -> level count, patches per level (the reference's order: coarsest level first).
tests/test_sampler_model.py holds the reference (through this file) and the device sampler's restatement to the same derived conditions.
skimage is only imported by the reference's module, never used on this path: a stub stands in when it is absent."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P = 16
K = 400
RAW = 8
SHAPES = [(32, 128, 4),(17, 40, 5), (64, 64, 10), (128, 160, 200), (288, 288, 300), (384, 512, 500)]        # (h, w, n) of one level
TABLE = [(h, w, count, ns, ratio, p)
         for (h, w) in [(16, 16), (17, 40), (40, 100), (64, 64), (80, 80), (45, 77), (160, 200), (301, 403), (384, 512), (1080, 1920)]
         for count in (3, 4, 30, 100, 500, 1024)
         for ns, ratio in ((1, 1.7), (2, 1.7), (3, 1.7), (4, 1.7), (3, 0.0), (3, 2.0))
         for p in (16, 8) if h >= p and w >= p and count >= ns]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "sampler_reference.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    try:
        import skimage.util.shape  # noqa: F401
    except ImportError:
        for name in ("skimage", "skimage.util", "skimage.util.shape"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["skimage.util.shape"].view_as_windows = None
    from data import patch_sampling as R

    out = {"shapes": np.asarray(SHAPES, np.int64), "K": np.int64(K), "P": np.int64(P)}
    sampler = R.PatchSampler()
    for i, (h, w, n) in enumerate(SHAPES):
        aspect = h / w
        wg = int(max(np.ceil(np.sqrt(n / aspect)), 1.))
        hg = int(np.ceil(wg * aspect))
        G = np.array([hg, wg], float).reshape(2, 1)
        ext = np.array([h - P, w - P], float).reshape(2, 1)
        np.random.seed(1000 + i)
        occupancy, offsets, raw = np.zeros((hg, wg), np.int64), np.zeros(2), []
        for k in range(K):
            s = sampler(h, w, P, P, num_samples=n)                   # float (2, n): rows, columns
            u = s / ext * G                                          # cell + 0.5 + jitter, jitter within +-0.4
            cell = np.floor(u).astype(np.int64)
            np.add.at(occupancy, (cell[0], cell[1]), 1)
            offsets += (u - cell).sum(axis=1)
            if k < RAW:
                raw.append(s)
        out[f"grid_{i}"] = np.array([hg, wg], np.int64)
        out[f"occupancy_{i}"] = occupancy
        out[f"offset_sum_{i}"] = offsets
        out[f"raw_{i}"] = np.stack(raw)
    levels, counts = [], np.zeros((len(TABLE), 4), np.int64)
    for j, (h, w, count, ns, ratio, p) in enumerate(TABLE):
        L = R.compute_patch_num_scales(ns, h, w, p, p)
        levels.append(L)
        counts[j, :L] = R.compute_num_patches_per_scale(count, L, ratio)
    out["table"] = np.asarray(TABLE, np.float64)
    out["table_levels"] = np.asarray(levels, np.int64)
    out["table_counts"] = counts
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
