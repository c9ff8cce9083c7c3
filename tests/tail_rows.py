"""The row counts at which the CLS tail and the DiffNet head change kernel form (tests/test_gpu_tail_rows.py), shared the way
tests/helpers.py is -- not a conftest.  Pure Python: tests/test_tail_rows_plan.py checks it without a GPU.

Both chains are skinny stages (skinny.hip) on one row per sequence: R = the call's sequence count in the tail, the number of scored
images in the head.  launch_skinny picks 16, 32 or 64 rows per workgroup -- three instantiations of skinny_linear_kernel -- and one or
several row workgroups (grid.y) from (R, N), so which code runs, and how far behind row R a workgroup reads the plane buffers
(R_pad, r_alloc of engine.hip), depends on the batch alone.  The catalogues below hold, for every output width N the chains launch, the
row counts on either side of each switch.
"""
from __future__ import annotations

CUS = 256                      # the grid that still "fits the CUs in one round" in launch_skinny's rule


def rows_per_workgroup(R: int, N: int) -> int:
    """skinny.hip launch_skinny (the four lines behind "Rows per workgroup"): `rb` row blocks of 16 per workgroup -- the first of 1, 2, 4
    with which the R rows fit ONE workgroup or the grid nb * ceil(R / (16 rb)) fits 256 CUs, else 4.  Returned in rows: 16, 32 or 64."""
    nb = (N + 15) // 16
    rb = 4
    for t in (1, 2, 4):
        if R <= 16 * t or nb * ((R + 16 * t - 1) // (16 * t)) <= CUS:
            rb = t
            break
    return 16 * rb


def row_workgroups(R: int, N: int) -> int:
    """grid.y of the same launch."""
    rows = rows_per_workgroup(R, N)
    return (R + rows - 1) // rows


def form(R: int, N: int):
    """(rows per workgroup, more than one row workgroup): what the tests want every value of, per width."""
    return rows_per_workgroup(R, N), row_workgroups(R, N) > 1


def possible_forms(N: int, horizon: int) -> set:
    """Every form the rule produces for width N at some R <= horizon."""
    return {form(R, N) for R in range(1, horizon + 1)}


def switches(N: int, horizon: int) -> list:
    """The row counts R < horizon behind which the form changes: R and R + 1 run different code."""
    return [R for R in range(1, horizon) if form(R, N) != form(R + 1, N)]


def catalogue(widths, horizon: int, beyond: int) -> list:
    """1, both sides of every switch of every width, and `beyond` (a count behind the last switch: a longer grid of the last form)."""
    out = {1, beyond}
    for N in widths:
        for R in switches(N, horizon):
            out |= {R, R + 1}
    return sorted(out)


# ---- the chains' widths (engine.hip run_encoder's tail block, run_head) ------------------------------------------------------

def tail_widths(H: int, mlp_dim: int) -> tuple:
    """Output widths of the tail's skinny stages: query, value and out projection, fc2 (H); fc1 (mlp_dim)."""
    return (H, mlp_dim)


def head_widths(H: int, ca_hidden: int) -> tuple:
    """Output widths of the head's stages: the RCAB conv with the CA squeeze folded in (H + ca_hidden), the CA gate / the residual
    groups' tail convs / the decoder's last conv (H), the predictor's two layers (H / 4, 1)."""
    return (H + ca_hidden, H, H // 4, 1)


# A tail call of G sequences of 8 patches is G * (8 + T) rows: 257 sequences (one count above 256, the issue of one workgroup per CU)
# stay at ~2,300 rows.  Behind TAIL_HORIZON the tail's widths have no further switch (test_tail_rows_plan.py pins that up to HEAD_HORIZON).
TAIL_HORIZON, TAIL_BEYOND = 256, 257
# The head's narrow stages switch late: N = H / 4 = 192 takes 32 rows per workgroup from 337 rows and 64 from 673.  The last stage (N = 1)
# would need 4097 rows to leave 16 rows per workgroup: more images than a test of seconds encodes, and the same instantiation the wider
# stages already run -- so the catalogue ends at HEAD_HORIZON and "every form" means every form up to there.
HEAD_HORIZON = 1024

VIT_B = dict(H=768, mlp_dim=3072, ca_hidden=96)          # spec.py: mlp_dim = 4 H, ca_hidden = H / ca_reduction (8)
VIT_L = dict(H=1024, mlp_dim=4096, ca_hidden=128)


def tail_catalogue(H: int, mlp_dim: int, **_) -> list:
    """Sequence counts G of the tail tests, ascending."""
    return catalogue(tail_widths(H, mlp_dim), TAIL_HORIZON, TAIL_BEYOND)


def head_catalogue(H: int, ca_hidden: int, **_) -> list:
    """Head batches (scored images M of forward_cached, HB of vtq_k_diffnet_head), ascending; the largest stays below HEAD_HORIZON."""
    return [R for R in catalogue(head_widths(H, ca_hidden), HEAD_HORIZON, 1) if R < HEAD_HORIZON]


def ragged_lengths(G: int, longest: int = 8) -> list:
    """Patch counts 1 .. longest in turn for the G images of a `lengths=` call."""
    return [1 + j % longest for j in range(G)]


def row_offsets(lengths, T: int) -> list:
    """Sequence j of a variable-length call is the rows [row0[j], row0[j] + lengths[j] + T) of the residual stream (engine.hip Table)."""
    out, r = [], 0
    for n in lengths:
        out.append(r)
        r += n + T
    return out
