"""The weighted device sampler's definition (include/vtamiq_hip_weighted_sampler.h) restated in numpy -- integers everywhere but the
allocation, which is fp64 with one numpy operation per rounding -- written from the header and independently of
csrc/patch_sampler_weighted.hip and of vtamiq_amd/sampling.py, and the catalogue of the smallest shapes at which the kernels can go wrong.
tests/test_weighted_sampler_model.py checks the restatement against the reference's recorded behaviour
(tests/golden/weighted_sampler_reference.npz); tests/test_gpu_weighted_sampler.py demands the kernels' bits equal it."""
import math
from collections import namedtuple

import numpy as np

from tests import sampler_model as SM

ACCEPT, DISSOLVE, ORDER, SUBCELL = 3, 4, 5, 6
MAX_CELLS = 8192
MAX_SAMPLES = 8100
MAX_PIXELS = 1 << 22
U64 = np.uint64
F = np.float64


# ---- 1: pixel weight and the pyramid (integers) ---------------------------------------------------------------------------------------------
def pixel_weight(a, b):
    """m_0 int64 (H, W) and (amin, amax, bmin, bmax) of a pair of HWC uint8 images."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    amin, amax, bmin, bmax = int(a.min()), int(a.max()), int(b.min()), int(b.max())
    Ra, Rb = amax - amin, bmax - bmin
    e = (a.astype(np.int64) - amin) * Rb - (b.astype(np.int64) - bmin) * Ra
    D = (e * e).sum(axis=2)
    r = np.floor(np.sqrt(D.astype(F))).astype(np.int64)
    r -= r * r > D
    r += (r + 1) * (r + 1) <= D
    assert ((r * r <= D) & ((r + 1) * (r + 1) > D)).all()
    return r, (amin, amax, bmin, bmax)


def pool(m0, level):
    """m_l: sums over the 2^l x 2^l blocks, the rows and columns behind (H >> l) 2^l dropped."""
    h, w = m0.shape[0] >> level, m0.shape[1] >> level
    s = 1 << level
    return m0[:h * s, :w * s].reshape(h, s, w, s).sum(axis=(1, 3))


# ---- 2: cells -----------------------------------------------------------------------------------------------------------------------------
def geometry(n, h, w, P):
    """(cs, sh, sw) in fp64 as numpy computes them in the reference (data/patch_sampling.py:240-253); sh, sw at least 1."""
    cs_d = np.sqrt(h * w / n * 4.)
    cs = int(max(0.75 * P, min(max(h, w) / P * 3., cs_d)))
    return cs, max(1, int(np.ceil((h - P) / cs))), max(1, int(np.ceil((w - P) / cs)))


def spans(dim, cs, s, P):
    """[(first, end)] of the s windows along an axis of `dim` pixels."""
    return [(j * cs, min(dim, j * cs + cs + P - 1)) for j in range(s)]


def window_areas(h, w, cs, sh, sw, P):
    rows = np.array([e - f for f, e in spans(h, cs, sh, P)], np.int64)
    cols = np.array([e - f for f, e in spans(w, cs, sw, P)], np.int64)
    return (rows[:, None] * cols[None, :]).reshape(-1)


def cell_sums(m, cs, sh, sw, P):
    h, w = m.shape
    return np.array([m[r0:r1, c0:c1].sum() for r0, r1 in spans(h, cs, sh, P) for c0, c1 in spans(w, cs, sw, P)], np.int64)


def extents(hm, cs, s):
    """The extent of every cell along one axis."""
    e = np.full(s, cs, np.int64)
    e[-1] = hm - (s - 1) * cs
    return e


def level_words(m, cs, sh, sw, P):
    """The 2 + sh sw table words of one level."""
    mu = m.astype(U64)
    return np.concatenate([np.array([mu.sum(), (mu * mu).sum()], U64), cell_sums(m, cs, sh, sw, P).astype(U64)])


def diff_table(pairs, levels, P):
    """pairs: [(a, b)] uint8 images; levels: per pair [(level, cs, sh, sw)].  Returns (tab uint64 [T], lev int32 [NL, 8], heads): the table
    vtq_k_diff_cells writes, the level rows it takes and every pair's head."""
    tab, lev, heads = [], [], []
    T = 0
    for p, ((a, b), rows) in enumerate(zip(pairs, levels)):
        m0, (amin, amax, bmin, bmax) = pixel_weight(a, b)
        head = T
        heads.append(head)
        tab.append(np.array([255 - amin, amax, 255 - bmin, bmax], U64))
        T += 4
        for level, cs, sh, sw in rows:
            lev.append((p, level, cs, sh, sw, head, T, 0))
            tab.append(level_words(pool(m0, level), cs, sh, sw, P))
            T += 2 + sh * sw
    return np.concatenate(tab), np.asarray(lev, np.int32).reshape(-1, 8), heads


def map_table(m, cs, sh, sw, P, Ra=255, Rb=255):
    """A one-level table (head at 0, level words at 4) for a given integer map m_l: what the tests hand the sampler as a synthetic table."""
    return np.concatenate([np.array([255, Ra, 255, Rb], U64), level_words(np.asarray(m, np.int64), cs, sh, sw, P)])


# ---- 3 and 4: allocation and placement ------------------------------------------------------------------------------------------------------
Segment = namedtuple("Segment", "samples cell k k_ceil use")      # int32 (n, 2); int64 (n,) flat cell of every sample; int64 (M,) counts; before the dissolve; bool


def allocation(n, h, w, level, cs, sh, sw, P, dw, uw, tab=None, head=-1, off=-1):
    """(k_c before the dissolve, `use`): the header's fp64 steps, one numpy operation per rounding."""
    M = sh * sw
    A = window_areas(h, w, cs, sh, sw, P)
    use = dw > 0 and tab is not None and head >= 0 and off >= 0
    S = np.zeros(M, U64)
    sd = F(0.0)
    if use:
        tab = np.asarray(tab, U64)
        Ra = int(tab[head + 1]) - (255 - int(tab[head])); Rb = int(tab[head + 3]) - (255 - int(tab[head + 2]))
        N = F(h * w)
        e1 = tab[off].astype(F) / N
        e2 = tab[off + 1].astype(F) / N
        var = e2 - e1 * e1
        if var < 0:
            var = F(0.0)
        sd = np.sqrt(var)
        use = bool(Ra > 0 and Rb > 0 and sd > F(1e-6) * F(Ra * Rb * 4 ** level))
        if use:
            S = tab[off + 2: off + 2 + M]
    SS, SA = U64(S.sum(dtype=U64)), U64(A.sum())
    d, u = (F(dw), F(uw) * sd) if use else (F(0.0), F(1.0))
    den = d * SS.astype(F) + u * SA.astype(F)
    if not den > 0:
        use, d, u, den, S = False, F(0.0), F(1.0), SA.astype(F), np.zeros(M, U64)
    x = (F(n) * (d * S.astype(F) + u * A.astype(U64).astype(F))) / den
    return np.clip(np.ceil(x), 0, n).astype(np.int64), use


def _ceil_sqrt(k):
    return np.array([math.isqrt(int(v) - 1) + 1 for v in k], np.int64)


def segment(seed, key, level, n, cs, sh, sw, hm, wm, P, q, dw, uw, tab=None, head=-1, off=-1):
    """One (image, level): n samples on sh x sw cells of size cs of a level with h - P = hm, w - P = wm."""
    M = sh * sw
    assert 1 <= n <= MAX_SAMPLES and 1 <= M <= MAX_CELLS and hm >= 0 and wm >= 0
    rng = lambda purpose, index: SM.rng(seed, key, level, purpose, index).astype(np.int64)
    k0, use = allocation(n, hm + P, wm + P, level, cs, sh, sw, P, dw, uw, tab, head, off)
    k = k0.copy()
    c = np.arange(M, dtype=np.int64)
    nz = c[k > 0]
    E = int(k.sum()) - n
    nE = min(abs(E), len(nz))
    if nE:
        cmax = int(k.max())
        preferred = rng(ACCEPT, nz) * cmax < ((cmax - k[nz]) << 32)
        first = nz[np.lexsort((nz, rng(DISSOLVE, nz), ~preferred))][:nE]
        k[first] += -1 if E > 0 else 1
    assert k.sum() == n, "the dissolve did not reach n"
    nz = c[k > 0]
    cells = nz[np.lexsort((nz, rng(ORDER, nz)))]
    kk = k[cells]
    first = np.cumsum(kk) - kk
    wd = _ceil_sqrt(kk)
    W2 = wd * wd
    assert W2.max() <= MAX_CELLS
    start = np.cumsum(W2) - W2
    slot = np.repeat(np.arange(len(cells)), W2)                      # the candidate sub-cells of all cells, cell after cell
    u = np.arange(W2.sum()) - np.repeat(start, W2)
    o = np.lexsort((u, rng(SUBCELL, cells[slot] * MAX_CELLS + u), slot))
    slot, u = slot[o], u[o]
    rank = np.arange(len(o)) - np.repeat(start, W2)
    take = rank < kk[slot]
    slot, u, rank = slot[take], u[take], rank[take]
    r = first[slot] + rank
    assert np.array_equal(r, np.arange(n))
    cell = cells[slot]
    j, i = cell // sw, cell % sw
    G = wd[slot]
    out = []
    for purpose, sub, base, ext, lim in ((SM.JITTER_ROW, u % G, j * cs, extents(hm, cs, sh)[j], hm), (SM.JITTER_COL, u // G, i * cs, extents(wm, cs, sw)[i], wm)):
        jitter = ((2 * (rng(purpose, r) >> 8) + 1 - (1 << 24)) * q) >> 15
        t = np.clip(sub * (1 << 24) + (1 << 23) + jitter, 0, G << 24)
        out.append(np.clip(base + np.clip(t * ext // (G << 24), 0, ext), 0, lim))
    return Segment(np.stack(out, axis=1).astype(np.int32), cell, k, k0, use)


# ---- the host arithmetic ------------------------------------------------------------------------------------------------------------------
def table(sizes, counts, num_scales, ratio, P):
    """[(image, first row, n, cs, sh, sw, h - P, w - P, level)] of a batch, level 0 first within an image, levels without patches left out."""
    out, first = [], 0
    for i, ((h, w), count) in enumerate(zip(sizes, counts)):
        L = SM.level_count(num_scales, h, w, P)
        for s, n in enumerate(SM.level_patches(count, L, ratio).tolist()):
            if n:
                out.append((i, first, n) + geometry(n, h >> s, w >> s, P) + ((h >> s) - P, (w >> s) - P, s))
                first += n
    return out


def pair_batch(refs, dists, counts, keys, seed, dw, uw, num_scales=1, ratio=1.7, P=16, amount=0.2, aligned=True):
    """What the pipeline samples for pairs of images: per-image lists (samples, scale_ids) for the references then the distorted images.
    aligned: both images of pair p get the rows of keys[p]; else the distorted image of pair p is drawn with keys[B + p] on the same table."""
    B = len(refs)
    counts = [counts] * B if np.ndim(counts) == 0 else list(counts)
    q = SM.amount_q(amount)
    smp, sid = [[] for _ in range(2 * B)], [[] for _ in range(2 * B)]
    sizes = [r.shape[:2] for r in refs]
    rows = table(sizes, counts, num_scales, ratio, P)
    levels = [[(s, cs, sh, sw) for i, _, _, cs, sh, sw, _, _, s in rows if i == p] for p in range(B)]
    tab, lev, heads = diff_table(list(zip(refs, dists)), levels, P)
    offs = {(int(r[0]), int(r[1])): int(r[6]) for r in lev}
    for side in range(2):
        for i, _, n, cs, sh, sw, hm, wm, s in rows:
            key = keys[i] if (aligned or side == 0) else keys[B + i]
            seg = segment(seed, key, s, n, cs, sh, sw, hm, wm, P, q, dw, uw, tab, heads[i], offs[(i, s)])
            smp[side * B + i].append(seg.samples)
            sid[side * B + i].append(np.full(n, s, np.int32))
    return [np.concatenate(x) for x in smp], [np.concatenate(x) for x in sid]


# ---- maps and images of the tests -----------------------------------------------------------------------------------------------------------
def hot_spot_map(h, w):
    """An integer difference map whose weight sits in 1/16 of the image: 1000 on rows [h/2, 3h/4) x columns [w/4, w/2), a ripple of 0 .. 49
    everywhere.  The golden recorder hands exactly this map to the reference as `diff`."""
    y, x = np.mgrid[0:h, 0:w]
    m = (7 * y + 13 * x) % 50
    m[h // 2: 3 * h // 4, w // 4: w // 2] += 1000
    return m.astype(np.int64)


def occupancy(samples, cs, sh, sw):
    """How many samples lie in every cell, a sample at (y, x) counted for cell (min(y // cs, sh - 1), min(x // cs, sw - 1)): the rule the
    recorder applies to the reference's real-valued samples (floor(floor(y) / cs) == floor(y / cs))."""
    j = np.minimum(np.asarray(samples)[:, 0].astype(np.int64) // cs, sh - 1)
    i = np.minimum(np.asarray(samples)[:, 1].astype(np.int64) // cs, sw - 1)
    return np.bincount(j * sw + i, minlength=sh * sw)


def image_pair(rs, h, w, lo_a=0, hi_a=255, lo_b=0, hi_b=255, spot=True):
    """A smooth-ish random reference with range [lo_a, hi_a] and a distorted copy with range [lo_b, hi_b] that differs in one region."""
    a = rs.randint(lo_a, hi_a + 1, size=(h, w, 3)).astype(np.int64)
    a[0, 0], a[-1, -1] = lo_a, hi_a
    b = (a - lo_a) * (hi_b - lo_b) // max(hi_a - lo_a, 1) + lo_b
    if spot:
        b[h // 3: h // 3 + max(h // 4, 1), w // 2: w // 2 + max(w // 4, 1)] = rs.randint(lo_b, hi_b + 1, size=b[h // 3: h // 3 + max(h // 4, 1), w // 2: w // 2 + max(w // 4, 1)].shape)
    b[0, 0], b[-1, -1] = lo_b, hi_b
    return a.astype(np.uint8), b.astype(np.uint8)
