"""The device sampler's definition (include/vtamiq_hip_sampler.h) restated in numpy -- int64 and uint32 only, written from the header and
independently of csrc/patch_sampler.hip and of vtamiq_amd/sampling.py -- and the catalogue of the smallest shapes at which the kernel can
go wrong.  tests/test_sampler_model.py checks the restatement against the reference's recorded behaviour (tests/golden/sampler_reference.npz);
tests/test_gpu_sampler.py demands the kernel's bits equal it."""
import math
from collections import namedtuple

import numpy as np

CELL, JITTER_ROW, JITTER_COL = 0, 1, 2
MAX_CELLS = 8192
U32 = np.uint32


def _rotl(x, r):
    return (x << U32(r)) | (x >> U32(32 - r))


def _absorb(h, k):
    """One 32-bit word into the MurmurHash3_x86_32 state; h, k uint32 arrays (array arithmetic wraps mod 2^32)."""
    k = _rotl(k * U32(0xcc9e2d51), 15) * U32(0x1b873593)
    return _rotl(h ^ k, 13) * U32(5) + U32(0xe6546b64)


def rng(seed, key, level, purpose, index):
    """uint32 array, one draw per entry of `index`: MurmurHash3_x86_32, seed 0, of (seed lo, seed hi, key lo, key hi, level, purpose, index)."""
    index = np.atleast_1d(np.asarray(index, dtype=np.int64)).astype(U32)
    seed, key = int(seed) % (1 << 64), int(key) % (1 << 64)
    h = np.zeros_like(index)
    for word in (seed & 0xffffffff, seed >> 32, key & 0xffffffff, key >> 32, level, purpose):
        h = _absorb(h, np.full_like(index, word))
    h = _absorb(h, index)
    h = h ^ U32(28)
    h = (h ^ (h >> U32(16))) * U32(0x85ebca6b)
    h = (h ^ (h >> U32(13))) * U32(0xc2b2ae35)
    return h ^ (h >> U32(16))


def amount_q(perturbed_amount):
    return int(round(perturbed_amount * 65536.0))


Segment = namedtuple("Segment", "samples cells jitter t")       # int32 (n, 2); int64 (n, 2) (row-cell, col-cell); int64 (n, 2); int64 (n, 2) unclamped


def segment(seed, key, level, n, Hg, Wg, hm, wm, q):
    """One (image, level): n samples on a grid of Hg x Wg cells of a level with h - P = hm, w - P = wm."""
    M = Hg * Wg
    assert 1 <= n <= M <= MAX_CELLS and hm >= 0 and wm >= 0
    c = np.arange(M, dtype=np.int64)
    order = np.lexsort((c, rng(seed, key, level, CELL, c).astype(np.int64)))          # by (draw, c) ascending
    chosen = order[:n]
    cells = np.stack([chosen % Hg, chosen // Hg], axis=1)
    r = np.arange(n, dtype=np.int64)
    bits = np.stack([rng(seed, key, level, JITTER_ROW, r) >> U32(8), rng(seed, key, level, JITTER_COL, r) >> U32(8)], axis=1).astype(np.int64)
    jitter = ((2 * bits + 1 - (1 << 24)) * q) >> 15
    t = cells * (1 << 24) + (1 << 23) + jitter
    G = np.array([Hg, Wg], np.int64)
    ext = np.array([hm, wm], np.int64)
    smp = np.clip(t, 0, G << 24) * ext // (G << 24)
    return Segment(np.clip(smp, 0, ext).astype(np.int32), cells, jitter, t)


# ---- the host arithmetic, from the reference's text (data/patch_sampling.py:308, 322-324, 398-447, 554-555) ---------------------------------
def level_count(num_scales, h, w, P):
    if num_scales <= 1:
        return 1
    d, k = float(min(h, w)), 0
    while d > 1:
        k, d = k + 1, (d - P) / 2
    return max(1, min(k - 1, num_scales))


def level_patches(patch_count, levels, ratio):
    """Counts per LEVEL, level 0 (full resolution) first: the reference's list reversed."""
    weights = np.power(2.0, ratio * np.arange(levels))
    num = np.ceil(weights * patch_count / weights.sum()).astype(np.int64)
    cum = np.cumsum(num)
    i = int(np.argmax(cum >= patch_count))
    num[i] -= cum[i] - patch_count
    num[i + 1:] = 0
    return num[::-1]


def grid(n, h, w):
    aspect = np.float64(h) / np.float64(w)
    wg = max(math.ceil(np.sqrt(np.float64(n) / aspect)), 1)
    return int(math.ceil(np.float64(wg) * aspect)), int(wg)


def table(sizes, counts, num_scales, ratio, P):
    """[(image, first row, n, Hg, Wg, h - P, w - P, level)] of a batch, level 0 first within an image, levels without patches left out."""
    out, first = [], 0
    for i, ((h, w), count) in enumerate(zip(sizes, counts)):
        L = level_count(num_scales, h, w, P)
        for s, n in enumerate(level_patches(count, L, ratio).tolist()):
            if n:
                out.append((i, first, n) + grid(n, h >> s, w >> s) + ((h >> s) - P, (w >> s) - P, s))
                first += n
    return out


def batch(sizes, counts, keys, seed, num_scales=1, ratio=1.7, P=16, amount=0.2):
    """(samples int32 (total, 2), scale_ids int32 (total,), lengths): what vtamiq_amd.sampling.sample_patches returns, image i with keys[i]."""
    counts = [counts] * len(sizes) if np.ndim(counts) == 0 else list(counts)
    q = amount_q(amount)
    smp, sid = [], []
    for i, first, n, Hg, Wg, hm, wm, s in table(sizes, counts, num_scales, ratio, P):
        smp.append(segment(seed, keys[i], s, n, Hg, Wg, hm, wm, q).samples)
        sid.append(np.full(n, s, np.int32))
    return np.concatenate(smp), np.concatenate(sid), [int(c) for c in counts]


def per_image(sizes, counts, keys, seed, num_scales=1, ratio=1.7, P=16, amount=0.2):
    """batch() split into per-image lists: what ImagePairVarlenPipeline.submit() takes as samples / scale_ids."""
    smp, sid, lengths = batch(sizes, counts, keys, seed, num_scales, ratio, P, amount)
    cut = np.cumsum(lengths)[:-1]
    return np.split(smp, cut), np.split(sid, cut)


# ---- the edge catalogue --------------------------------------------------------------------------------------------------------------------
# name, (H, W), patch_count, num_scales, ratio, P, amount; `expect` pins what makes the case an edge: (level, n, Hg, Wg) of its segments
Case = namedtuple("Case", "name size count num_scales ratio P amount expect")


def _c(name, size, count, expect, num_scales=1, ratio=1.7, P=16, amount=0.2):
    return Case(name, size, count, num_scales, ratio, P, amount, expect)


CATALOGUE = [
    _c("n = 1, M = 1", (64, 64), 1, [(0, 1, 1, 1)]),
    _c("n = M: every cell taken", (64, 64), 16, [(0, 16, 4, 4)]),
    _c("Hg = 1", (16, 64), 4, [(0, 4, 1, 4)]),
    _c("Wg = 1", (64, 16), 3, [(0, 3, 4, 1)]),
    _c("image of exactly P x P: every sample 0", (16, 16), 5, [(0, 5, 3, 3)]),
    _c("h - P = 1", (17, 40), 5, [(0, 5, 2, 4)]),
    _c("odd dimensions at levels 1 - 3", (301, 403), 100, [(0, 68, 8, 10), (1, 22, 5, 6), (2, 7, 3, 4), (3, 3, 3, 3)], num_scales=4),
    _c("M = 63", (112, 144), 60, [(0, 60, 7, 9)]),
    _c("M = 64", (64, 64), 50, [(0, 50, 8, 8)]),
    _c("M = 65", (80, 208), 60, [(0, 60, 5, 13)]),
    _c("M = 255", (240, 272), 250, [(0, 250, 15, 17)]),
    _c("M = 256 = n: the last grid of the four-wave launch", (64, 64), 256, [(0, 256, 16, 16)]),
    _c("M = 272, n = 257: the first of the sixteen-wave launch", (128, 136), 257, [(0, 257, 16, 17)]),
    _c("n = 255", (64, 64), 255, [(0, 255, 16, 16)]),
    _c("n = 511", (64, 128), 511, [(0, 511, 16, 32)]),
    _c("n = 512 = M", (64, 128), 512, [(0, 512, 16, 32)]),
    _c("n = 513", (64, 128), 513, [(0, 513, 17, 33)]),
    _c("n = 1023", (64, 64), 1023, [(0, 1023, 32, 32)]),
    _c("n = 1024 = M: one cell per thread of the sixteen-wave launch", (64, 64), 1024, [(0, 1024, 32, 32)]),
    _c("n = 1025", (64, 64), 1025, [(0, 1025, 33, 33)]),
    _c("M = 2048 = n: two cells per thread of the sixteen-wave launch", (64, 128), 2048, [(0, 2048, 32, 64)]),
    _c("M = 2145: a third cell for some threads", (64, 128), 2049, [(0, 2049, 33, 65)]),
    _c("M = 8192: the limit", (64, 128), 8192, [(0, 8192, 64, 128)]),
    _c("N = 5000 on 384 x 512", (384, 512), 5000, [(0, 5000, 62, 82)]),
    _c("three scales asked, one level by the reference's rule", (40, 100), 30, [(0, 30, 4, 9)], num_scales=3),
    _c("three scales asked, two levels", (80, 80), 30, [(0, 22, 5, 5), (1, 8, 3, 3)], num_scales=3),
    _c("three scales, three levels", (160, 200), 30, [(0, 20, 4, 5), (1, 7, 3, 3), (2, 3, 2, 2)], num_scales=3),
    _c("patch_count 3 on three scales: 1 / 1 / 1", (160, 200), 3, [(0, 1, 2, 2), (1, 1, 2, 2), (2, 1, 2, 2)], num_scales=3),
    _c("equal split of 4 over three scales: level 0 stays empty", (160, 200), 4, [(1, 2, 2, 2), (2, 2, 2, 2)], num_scales=3, ratio=0.0),
    _c("amount 0: cell centres", (96, 128), 40, [(0, 40, 6, 8)], amount=0.0),
    _c("amount 0.5: jitter of a whole cell reaches the clamp", (96, 128), 40, [(0, 40, 6, 8)], amount=0.5),
    _c("amount 0.5 on one cell row", (16, 64), 4, [(0, 4, 1, 4)], amount=0.5),
    _c("amount 0.5, three levels", (160, 200), 30, [(0, 20, 4, 5), (1, 7, 3, 3), (2, 3, 2, 2)], num_scales=3, amount=0.5),
    # P = 8
    _c("P = 8: image of exactly P x P", (8, 8), 3, [(0, 3, 2, 2)], P=8),
    _c("P = 8: h - P = 1", (9, 20), 5, [(0, 5, 2, 4)], P=8),
    _c("P = 8: n = M", (64, 64), 16, [(0, 16, 4, 4)], P=8),
    _c("P = 8: Hg = 1", (8, 32), 4, [(0, 4, 1, 4)], P=8),
    _c("P = 8: three levels where P = 16 has two", (80, 80), 30, [(0, 20, 5, 5), (1, 7, 3, 3), (2, 3, 2, 2)], num_scales=3, P=8),
    _c("P = 8: odd dimensions, amount 0.5", (45, 77), 257, [(0, 257, 13, 21)], P=8, amount=0.5),
]
# refused: the plan (ValueError) and, as a raw table, the entry
OVER_LIMIT = _c("M = 8385: above the limit", (64, 128), 8193, [(0, 8193, 65, 129)])


def case_table(case):
    return table([case.size], [case.count], case.num_scales, case.ratio, case.P)


def case_segments(case, seed, key):
    return [segment(seed, key, s, n, Hg, Wg, hm, wm, amount_q(case.amount)) for _, _, n, Hg, Wg, hm, wm, s in case_table(case)]
