"""What tests/test_gpu_interleave.py relies on, checked on the host (tests/interleave.py): the plan holds every ordered pair of entry
kinds and every catalogue entry, it goes small -> large -> small for both workspaces, and every poisoned carrier call covers the slack
rows of every clean call that is run behind it.  They fail here, without a GPU, when someone edits the catalogue."""
from tests import interleave as il


def test_euler_walk_uses_every_ordered_pair_once():
    for n in (1, 2, 3, 8):
        walk = il.euler_walk(n)
        steps = list(zip(walk, walk[1:]))
        assert len(walk) == n * n + 1 and walk[0] == walk[-1] == 0
        assert sorted(steps) == [(i, j) for i in range(n) for j in range(n)]


def test_plan_covers_every_ordered_pair_of_kinds_and_every_entry():
    plan = il.plan()
    assert plan == il.plan()                                               # deterministic
    assert 65 <= len(plan) <= 85
    kinds = [il.CATALOGUE[n].kind for n in plan]
    assert set(zip(kinds, kinds[1:])) == {(a, b) for a in il.KINDS for b in il.KINDS}
    assert set(plan) == set(il.CATALOGUE)
    assert len(il.KINDS) == 8 and {il.CATALOGUE[n].kind for n in il.SMALL} == set(il.KINDS)


def _small_large_small(sizes):
    """Does the sequence hold a small call, later a large one, later a small one?"""
    if "small" not in sizes:
        return False
    first = sizes.index("small")
    if "large" not in sizes[first:]:
        return False
    return "small" in sizes[first + sizes[first:].index("large"):]


def test_plan_shrinks_behind_a_large_call_in_both_workspaces():
    plan = [il.CATALOGUE[n] for n in il.plan()]
    assert plan[0].size == "small"                                         # the engine's first workspace is a small one
    assert _small_large_small([e.size for e in plan])
    assert _small_large_small([e.size for e in plan if e.kind == "rollout"])
    # and in rows, as the engine counts them: a call below the high-water mark of the calls in front of it, for both workspaces
    for calls in (plan, [e for e in plan if e.kind == "rollout"]):
        high = 0
        shrunk = False
        for e in calls:
            shrunk |= e.m_pad < high
            high = max(high, e.m_pad)
        assert shrunk


def test_geometry_restates_the_engine():
    assert il.seq_rows(6, 40) == 252 and il.ceil256(252) == 256            # the pairwise triplets: 4 rows short of the GEMM tile
    assert il.ceil256(256) == 256 and il.ceil256(257) == 512 and il.ceil256(1) == 256
    assert il.varlen_rows([8, 130, 63]) == 2 * (201 + 3 * il.T) == 414
    # the small calls that are there to read the slack rows behind M_pad: their last sequence's 64-key tiles end past it
    for name, last_len in (("pairwise_small", 40 + il.T), ("rollout_small", 40 + il.T), ("varlen_small", il.VL_SMALL[-1] + il.T)):
        e = il.CATALOGUE[name]
        start = e.rows[0] - last_len
        assert e.m_pad < start + (last_len + 63) // 64 * 64 <= e.m_pad + il.SLACK_ROWS, name
    assert il.CATALOGUE["cached_small"].rows == [84, 237] and il.CATALOGUE["cached_small"].m_pad == 256
    assert il.spec().num_tokens == il.T


def test_every_carrier_covers_the_slack_rows_of_every_clean_call():
    """A carrier makes rows [0, rows) of the workspace non-finite.  The clean call behind it reads rows [M_pad, M_pad + 128) of the QKV
    buffer as masked keys: those must be rows the carrier wrote, or the test would pass over zeros."""
    for c in il.CARRIERS:
        carrier = il.CATALOGUE[c]
        assert carrier.size == "large" and len(carrier.rows) == 1
        for n in il.SMALL:
            clean = il.CATALOGUE[n]
            assert carrier.rows[0] >= clean.m_pad + il.SLACK_ROWS, (c, carrier.rows[0], n, clean.m_pad)
    assert {il.CATALOGUE[c].kind for c in il.CARRIERS} == {"forward", "rollout", "varlen", "group", "vit"}


def test_poison_offsets_stay_inside_their_pair():
    for name, lengths in (("varlen_small", il.VL_SMALL), ("varlen_large", il.VL_LARGE)):
        e = il.CATALOGUE[name]
        assert len(e.offsets) == len(lengths)
        for off, n, nxt in zip(e.offsets, lengths, e.offsets[1:] + [sum(lengths)]):
            assert off + 1 < off + n == nxt
