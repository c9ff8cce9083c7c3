"""The seam inputs of tests/attention_seams.py discriminate: at every seam length an off-by-one key mask moves every query row of the fp64
answer by at least 10 x the loosest bound tests/test_gpu_attention_seams.py compares a kernel with.  Runs on the CPU, 2 heads, fp64; this is
the proof that the GPU tests can fail.  The smallest distances are printed per kernel family (pytest -s)."""
import functools

import torch

from tests import attention_seams as A

NH = 2
# 10 x the loosest bound of the GPU file: PROBS_TOL[False] = 2e-3 absolute (probs, rollout step), ATTN_TOL["bf16"] = 1.5e-2 of max |ref|
PROBS_MIN, ROLLOUT_MIN, ATTN_MIN = 2e-2, 2e-2, 0.15
LAYOUTS = ("packed", "padded", "last")


@functools.lru_cache(maxsize=None)
def case(S, layout):
    """(fp64 values (rows, 3H), first row of the sequence under test: one of three of length S).  packed: the middle one, the row behind S - 1 is
    the next sequence's row 0; padded: the middle one at pitch = S rounded up to 32, pad rows behind S - 1 (none at a multiple of 32); last: the
    sequence in front of the slack rows."""
    base, u = A.base_rows(NH, 3 * 544 + A.SLACK, 99)
    pitch = (S + 31) // 32 * 32 if layout == "padded" else S
    qkv = A.make_qkv([S] * 3, [pitch] * 3, base, u).double()
    return qkv, (2 if layout == "last" else 1) * pitch


def sweep(distance, floor, family, exempt=()):
    """distance(val, r0, S, variant) -> per-row (or per-vector) distances of the wrong variant from the truth; every one of them >= floor."""
    misses, smallest = [], {w: (float("inf"), None) for w in A.WRONG}
    for S in A.SEAMS:
        for layout in LAYOUTS:
            val, r0 = case(S, layout)
            for w in A.WRONG:
                if (S, w) in exempt:
                    continue
                d = distance(val, r0, S, w)
                lo, at = float(d.min()), int(d.argmin())
                if lo < smallest[w][0]:
                    smallest[w] = (lo, (S, layout, at))
                if not lo >= floor:
                    misses.append((S, layout, w, at, lo))
    for w in A.WRONG:
        print(f"smallest off-by-one distance, {family}, {w}: {smallest[w][0]:.3g} at (S, layout, row) = {smallest[w][1]}   (floor {floor})")
    assert not misses, misses


def test_the_generator_is_what_the_docstring_says():
    base, u = A.base_rows(NH, 3 * 544 + A.SLACK, 99)
    H = NH * 64
    assert torch.allclose(u.norm(dim=-1), torch.ones(NH))
    lengths, pitches = [5, 33, 1], [32, 64, 1]
    qkv = A.make_qkv(lengths, pitches, base, u)
    starts, rows = A.starts_of(lengths, pitches)
    assert starts == [0, 32, 96] and rows == 97 and qkv.shape == (97 + A.SLACK, 3 * H)
    assert torch.equal(qkv[:, 2 * H:], base[:97 + A.SLACK, 2 * H:])                      # V is the base draw
    spikes = sorted({0, *range(4, 32), 32, *range(64, 96), 96, *range(97, 97 + A.SLACK)})
    plain = [r for r in range(97 + A.SLACK) if r not in spikes]
    assert torch.equal(qkv[plain, H:2 * H], base[plain, H:2 * H])
    k = qkv[spikes, H:2 * H].view(-1, NH, 64)
    assert float(((k * u).sum(-1) - A.SPIKE).abs().max()) < 0.1 * 0.5 * 5                # b u_h plus a tenth of a base row
    q = (qkv[:97, :H] - base[:97, :H]).view(97, NH, 64)
    want = torch.cat([torch.full((p,), 8.0 * (torch.log(torch.tensor(float(s))) + A.MARGIN) / A.SPIKE) for s, p in zip(lengths, pitches)])
    assert torch.allclose((q * u).sum(-1), want[:, None].expand(97, NH), atol=1e-5)
    assert torch.equal(qkv[97:, :H], base[97:97 + A.SLACK, :H])                          # slack rows: no query bump
    assert torch.equal(A.make_qkv(lengths, pitches, base, u), qkv) and torch.equal(A.base_rows(NH, 3 * 544 + A.SLACK, 99)[0], base)


def test_boundary_keys_dominate_and_logits_stay_moderate():
    for S in A.SEAMS:
        val, r0 = case(S, "packed")
        P = A.probs_ref(val, r0, S)
        last = P[:, :, S - 1]
        if S > 1:
            assert 0.25 <= float(last.min()) and float(last.max()) <= 0.55, (S, float(last.min()), float(last.max()))
        H = NH * 64
        q = val[r0:r0 + S, :H].view(S, NH, 64).permute(1, 0, 2)
        k = val[r0:r0 + S + 1, H:2 * H].view(S + 1, NH, 64).permute(1, 0, 2)
        assert float((q @ k.transpose(-1, -2) / 8.0).abs().max()) < 9.5, S


def test_every_partial_wave_tile_and_block_has_a_row_under_test():
    """The distances below are taken on EVERY query row of a sequence, so the rows of its last partial wave, key tile and query block are among
    them; this states it per length, and that every granule has a length below, at and above a multiple of it."""
    for S in A.SEAMS:
        val, r0 = case(S, "packed")
        d = A.row_distance(A.probs_ref(val, r0, S, "drop_last"), A.probs_ref(val, r0, S))
        assert d.shape == (NH, S)
        for g in A.GRANULES:
            if S % g:
                tail = d[:, S // g * g:]
                assert tail.shape[1] == S % g and bool((tail >= PROBS_MIN).all()), (S, g)
    for g in A.GRANULES:
        rem = {S % g for S in A.SEAMS if S >= g - 1}
        assert {g - 1, 0, 1} <= rem, (g, rem)


def test_probs_of_a_wrong_mask_differ_on_every_row():
    sweep(lambda val, r0, S, w: A.row_distance(A.probs_ref(val, r0, S, w), A.probs_ref(val, r0, S)), PROBS_MIN, "probs")


def test_attention_of_a_wrong_mask_differs_on_every_row():
    def distance(val, r0, S, w):
        ref = A.attention_ref(val, r0, S)
        return A.row_distance(A.attention_ref(val, r0, S, w), ref) / ref.abs().max()
    # S = 1: a weighted mean over one key twice is that key's V row, as the true answer is.  No input can show it in the OUTPUT; the
    # probabilities (1/2 instead of 1) and the rollout step show it, and those are the kernels that clamp their loads to row S - 1.
    sweep(distance, ATTN_MIN, "attention output (of the sequence's max |ref|)", exempt={(1, "count_last_twice")})


def test_rollout_of_a_wrong_mask_differs_for_every_r():
    def distance(val, r0, S, w):
        r = A.rollout_inputs(S)
        return A.row_distance(A.rollout_ref(r, A.probs_ref(val, r0, S, w)), A.rollout_ref(r, A.probs_ref(val, r0, S)))     # one per r_in
    sweep(distance, ROLLOUT_MIN, "rollout step (random r, one-hot S-1, one-hot 0)")
