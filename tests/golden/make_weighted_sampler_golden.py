"""Records how the reference's difference-weighted patch sampler behaves -> tests/golden/weighted_sampler_reference.npz (recorded results
and three tiny image pairs only).

    python tests/golden/make_weighted_sampler_golden.py --reference /path/to/the/reference/checkout

Runs the reference's PatchSampler(grid_type=GRID_TYPE_PERTURBED, diff_weight, uniform_weight) under fixed numpy seeds:
  per (shape, weighting), with tests/weighted_sampler_model.hot_spot_map(h, w) as `diff`: two independent records A and B of K = 400 calls
  each -- how many samples fell in every cell (a sample counted for the cell floor(coordinate / cell size), clipped to the last cell) and
  the sums of the in-cell offsets -- and the first eight calls of A raw;
  per tiny uint8 pair stored in the file, per level: the cell probabilities the reference derives through compute_diff at
  uniform_weight = 0 (the normalised window sums of stratified_grid_sampling, taken where it computes them).
skimage is absent where this ran: numpy's sliding_window_view stands in for its view_as_windows, and the stand-in is also where the cell
probabilities are read.  tests/test_weighted_sampler_model.py holds the restatement of the device sampler to these records."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import weighted_sampler_model as WM  # noqa: E402

P = 16
K = 400
RAW = 8
SHAPES = [(384, 512, 500), (288, 288, 300), (192, 256, 110), (64, 80, 24)]      # (h, w, n) of one level
WEIGHTS = [(1.0, 0.1), (1.0, 1.0)]                                                # (diff_weight, uniform_weight)
PAIR_COUNTS = [[12], [10], [20, 8, 4]]                                           # samples per level of the three pairs


def make_pairs():
    rs = np.random.RandomState(77)
    return [WM.image_pair(rs, 40, 56, 0, 255, 0, 255),
            WM.image_pair(rs, 48, 48, 10, 250, 30, 235),                          # Ra = 240, Rb = 205
            WM.image_pair(rs, 71, 85, 3, 255, 0, 222)]                            # odd at every level, three levels; Ra = 252, Rb = 222


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "weighted_sampler_reference.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    seen = []

    def view_as_windows(arr, shape, step):
        win = np.lib.stride_tricks.sliding_window_view(arr, shape)[::step[0], ::step[1]]
        sums = win.sum(axis=(2, 3))
        seen.append(sums / sums.sum())
        return win

    try:
        import skimage.util.shape  # noqa: F401
    except ImportError:
        for name in ("skimage", "skimage.util", "skimage.util.shape"):
            sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.util.shape"].view_as_windows = view_as_windows
    import torch
    from data import patch_sampling as R
    R.view_as_windows = view_as_windows

    out = {"shapes": np.asarray(SHAPES, np.int64), "weights": np.asarray(WEIGHTS, np.float64), "K": np.int64(K), "P": np.int64(P)}
    for i, (h, w, n) in enumerate(SHAPES):
        cs, sh, sw = WM.geometry(n, h, w, P)
        diff = WM.hot_spot_map(h, w).astype(float)
        for v, (dw, uw) in enumerate(WEIGHTS):
            sampler = R.PatchSampler(diff_weight=dw, uniform_weight=uw, grid_type=R.GRID_TYPE_PERTURBED)
            for rec in "AB":
                np.random.seed(5000 + 100 * i + 10 * v + (rec == "B"))
                occ, offsets, raw = np.zeros(sh * sw, np.int64), np.zeros(2), []
                for k in range(K):
                    s = sampler(h, w, P, P, diff=diff, num_samples=n)        # float (2, n): rows, columns
                    assert seen[-1].shape == (sh, sw)
                    cell = np.minimum(np.floor(s / cs).astype(np.int64), np.array([[sh - 1], [sw - 1]]))
                    occ += np.bincount(cell[0] * sw + cell[1], minlength=sh * sw)
                    offsets += (s / cs - cell).sum(axis=1)
                    if k < RAW and rec == "A":
                        raw.append(s)
                out[f"occupancy_{rec}_{i}_{v}"] = occ
                out[f"offset_sum_{rec}_{i}_{v}"] = offsets
                if rec == "A":
                    out[f"raw_{i}_{v}"] = np.stack(raw)
        out[f"cells_{i}"] = np.array([cs, sh, sw], np.int64)

    sampler = R.PatchSampler(diff_weight=1.0, uniform_weight=0.0, grid_type=R.GRID_TYPE_PERTURBED)
    pool = torch.nn.AvgPool2d(kernel_size=2)
    for p, ((ia, ib), counts) in enumerate(zip(make_pairs(), PAIR_COUNTS)):
        out[f"pair_{p}_a"], out[f"pair_{p}_b"] = ia, ib
        out[f"pair_{p}_counts"] = np.asarray(counts, np.int64)
        diff = sampler.compute_diff([ia, ib])
        for level, n in enumerate(counts):
            h, w = diff.shape
            np.random.seed(9000 + 10 * p + level)
            sampler(h, w, P, P, diff=diff, num_samples=n)
            out[f"pair_{p}_prob_{level}"] = seen[-1]
            out[f"pair_{p}_cells_{level}"] = np.array((WM.geometry(n, h, w, P)), np.int64)
            assert seen[-1].shape == tuple(out[f"pair_{p}_cells_{level}"][1:])
            diff = pool(torch.as_tensor(diff).view(1, 1, *diff.shape)).squeeze().numpy()
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
