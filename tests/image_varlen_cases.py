"""Cases and CPU references shared by tests/test_image_varlen_layout.py and tests/test_gpu_image_varlen.py: batches of images of different
sizes with patches at the corners of every pyramid level that holds one, and the oracle (oracle/patch_oracle.py) composed per image."""
import numpy as np
import torch

from oracle import patch_oracle as PO

# (H, W), patches: the smallest shapes at which the ragged gather can go wrong -- one position only (16 x 16), odd dimensions whose byte
# count is odd (17 x 33 = 1683 bytes: everything behind starts at an odd address), levels that drop a row / column (37 x 53 -> 18 x 26,
# 64 x 67 -> 32 x 33 -> 16 x 16: one position at level 2), and an image of several hundred positions
SIZES = [(16, 16), (17, 33), (37, 53), (64, 67), (96, 128)]
COUNTS = [1, 2, 5, 9, 60]
NUM_SCALES = 3
ROUNDS = 5          # turns of make_samples / flips_of_turn after which every corner of every level and every flip combination has occurred


def levels_with_a_patch(h, w, num_scales, P):
    return [s for s in range(num_scales) if (h >> s) >= P and (w >> s) >= P]


def corners(h, w, s, P):
    """The four corner positions of level s (fewer where they coincide)."""
    hm, wm = (h >> s) - P, (w >> s) - P
    return sorted({(0, 0), (0, wm), (hm, 0), (hm, wm)})


def make_samples(sizes, counts, num_scales, P, seed, turn=0):
    """Per image: int32 samples (n, 2) and scale ids (n,): corners of the levels that hold a patch first -- all of them where the count
    allows, else a window of the list that moves with `turn`, so that ROUNDS turns cover every corner -- then seeded random positions on
    random levels."""
    rs = np.random.RandomState(seed + 1000 * turn)
    smp, sid = [], []
    for (h, w), n in zip(sizes, counts):
        lv = levels_with_a_patch(h, w, num_scales, P)
        every = [(r, c, s) for s in reversed(lv) for r, c in corners(h, w, s, P)]
        rows = every if len(every) <= n else [every[(turn * n + k) % len(every)] for k in range(n)]
        while len(rows) < n:
            s = lv[rs.randint(len(lv))]
            rows.append((rs.randint(0, (h >> s) - P + 1), rs.randint(0, (w >> s) - P + 1), s))
        a = np.asarray(rows, dtype=np.int32).reshape(n, 3)
        smp.append(np.ascontiguousarray(a[:, :2]))
        sid.append(np.ascontiguousarray(a[:, 2]))
    return smp, sid


def flips_of_turn(n_images, turn):
    """(hflip, vflip) per image: image k sees all four combinations over four turns."""
    return [((k + turn) & 1, ((k + turn) >> 1) & 1) for k in range(n_images)]


def make_images(sizes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def oracle_image(img, smp, sid, num_scales, flip=(0, 0), P=16, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """oracle.patch_oracle on ONE image, rows in the order of smp / sid: patches (n, 3, P, P), pos (n, 2), scales (n,) fp32 or None."""
    t = PO.transform_img(img, bool(flip[0]), bool(flip[1]), mean, std)
    order = [np.nonzero(sid == s)[0] for s in range(num_scales)]
    deepest = max(s for s in range(num_scales) if len(order[s])) + 1           # the oracle pools once per listed scale
    pa, po, sc = PO.extract_patches([t], [[smp[order[s]].T.astype(np.int64)] for s in range(deepest)], P)
    back = np.argsort(np.concatenate(order[:deepest]), kind="stable")
    scales = torch.from_numpy(sid.astype(np.float32)) if num_scales > 1 else None
    return pa[0][back].contiguous(), po[0][back].contiguous(), scales


def oracle_batch(images, smp, sid, num_scales, flips=None, P=16):
    """The per-image oracle outputs concatenated in image order."""
    outs = [oracle_image(im, s, i, num_scales, flips[k] if flips is not None else (0, 0), P) for k, (im, s, i) in enumerate(zip(images, smp, sid))]
    return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]),
            torch.cat([o[2] for o in outs]) if num_scales > 1 else None)
