"""The row-count catalogues of tests/tail_rows.py cover every form launch_skinny's rule produces (no GPU needed).

If the rule in skinny.hip changes, tail_rows.rows_per_workgroup must change with it (the first test reads the source), and then the
coverage tests say whether the catalogues still reach every form."""
import os
import re

import pytest

from tests import tail_rows as R

CONFIGS = {"ViT-B": R.VIT_B, "ViT-L": R.VIT_L}
SKINNY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vtamiq_amd", "csrc", "skinny.hip")


def test_rule_is_the_one_in_skinny_hip():
    """The restated rule, line by line, against the launcher's text: a change of the source fails here first."""
    src = re.sub(r"\s+", " ", open(SKINNY).read())
    for line in ("const int nb = (a.N + 15) / 16;",
                 "int rb = 4;",
                 "for (int t = 1; t <= 4; t *= 2)",
                 "if (a.R <= 16 * t || nb * ((a.R + 16 * t - 1) / (16 * t)) <= 256) { rb = t; break; }",
                 "const dim3 g(nb, (a.R + 16 * rb - 1) / (16 * rb)), blk(512);"):
        assert line in src, line


def test_rule_values():
    """Hand-computed: N = 768 is 48 channel workgroups, so 5 row workgroups fit 256 CUs; N = 3072 is 192, so one does."""
    assert [R.rows_per_workgroup(r, 768) for r in (1, 16, 17, 80, 81, 160, 161, 320, 321, 5000)] == [16, 16, 16, 16, 32, 32, 64, 64, 64, 64]
    assert [R.row_workgroups(r, 768) for r in (1, 16, 17, 80, 81, 160, 161, 257)] == [1, 1, 2, 5, 3, 5, 3, 5]
    assert [R.rows_per_workgroup(r, 3072) for r in (1, 16, 17, 32, 33, 64, 65, 257)] == [16, 16, 32, 32, 64, 64, 64, 64]
    assert [R.row_workgroups(r, 3072) for r in (16, 17, 32, 33, 64, 65, 257)] == [1, 1, 1, 1, 1, 2, 5]
    assert R.rows_per_workgroup(4096, 1) == 16 and R.rows_per_workgroup(4097, 1) == 32


def _covered(widths, counts, horizon):
    missing = []
    for N in widths:
        have = {R.form(r, N) for r in counts}
        missing += [(N, f) for f in sorted(R.possible_forms(N, horizon) - have)]
    return missing


@pytest.mark.parametrize("name", CONFIGS)
def test_tail_catalogue_reaches_every_form(name):
    c = CONFIGS[name]
    widths, counts = R.tail_widths(c["H"], c["mlp_dim"]), R.tail_catalogue(**c)
    # the horizon of the claim is the head's (1024 rows), four times the catalogue's own: no form of a tail width first appears behind 257
    assert _covered(widths, counts, R.HEAD_HORIZON) == []
    for N in widths:                                   # both sides of every switch, 1 and a count above 256
        for s in R.switches(N, R.HEAD_HORIZON):
            assert s in counts and s + 1 in counts, (N, s)
    assert counts[0] == 1 and counts[-1] > 256 and counts == sorted(set(counts))
    # 16, 32 and 64 rows per workgroup each with one row workgroup and with several, wherever the rule can produce the combination
    forms = {R.form(r, N) for N in widths for r in counts}
    assert forms == {(16, False), (16, True), (32, False), (32, True), (64, False), (64, True)}


@pytest.mark.parametrize("name", CONFIGS)
def test_head_catalogue_reaches_every_form(name):
    c = CONFIGS[name]
    widths, counts = R.head_widths(c["H"], c["ca_hidden"]), R.head_catalogue(**c)
    assert _covered(widths, counts, R.HEAD_HORIZON) == []
    for N in widths:
        for s in R.switches(N, R.HEAD_HORIZON):
            assert s in counts and s + 1 in counts, (N, s)
    assert counts[0] == 1 and counts[-1] < R.HEAD_HORIZON
    # the head has no width of a single channel workgroup row that is wide enough for 32 / 64 rows in ONE row workgroup (that takes
    # nb > 128: the tail's fc1); every other combination appears
    forms = {R.form(r, N) for N in widths for r in counts}
    assert forms == {(16, False), (16, True), (32, True), (64, True)}
    # beyond the horizon only the last stage (N = 1) changes form, at 4097 rows (tail_rows.py says why the catalogue stops before)
    late = {N: [s for s in R.switches(N, 8192) if s >= R.HEAD_HORIZON] for N in widths}
    assert late == {N: ([4096] if N == 1 else []) for N in widths}


def test_catalogues_as_read_from_the_rule():
    """The lists the GPU tests walk, written out: a reviewer sees here what a change of the rule did to them."""
    assert R.tail_catalogue(**R.VIT_B) == [1, 16, 17, 32, 33, 64, 65, 80, 81, 160, 161, 257]
    assert R.tail_catalogue(**R.VIT_L) == [1, 16, 17, 32, 33, 64, 65, 128, 129, 257]
    assert R.head_catalogue(**R.VIT_B) == [1, 16, 17, 64, 65, 80, 81, 128, 129, 160, 161, 336, 337, 672, 673]
    assert R.head_catalogue(**R.VIT_L) == [1, 16, 17, 48, 49, 64, 65, 96, 97, 128, 129, 256, 257, 512, 513]


def test_configs_match_the_specs():
    from vtamiq_amd.spec import make_spec
    for variant, c in (("ViT-B16", R.VIT_B), ("ViT-L16", R.VIT_L)):
        spec = make_spec(vit_config=dict(variant=variant, pretrained=False))
        assert (spec.hidden_size, spec.mlp_dim, spec.ca_hidden) == (c["H"], c["mlp_dim"], c["ca_hidden"])


def test_ragged_layout():
    lens = R.ragged_lengths(81)
    assert len(lens) == 81 and set(lens) == set(range(1, 9)) and lens[:9] == [1, 2, 3, 4, 5, 6, 7, 8, 1]
    assert R.row_offsets([3, 1, 2], 9) == [0, 12, 22]
