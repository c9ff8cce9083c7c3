"""The per-row comparator and the workspace decoders of tests/stage_probe.py, on the CPU: the stage checks of tests/test_gpu_stages.py
can only catch a corrupted row if the comparator sees one that a whole-tensor metric does not, and only check the right rows if the
layouts of DESIGN.md section 3 are decoded the way the engine writes them."""
import math

import pytest
import torch

from tests.stage_probe import StageLog, StageProbe, global_error, row_error, worst_row

BOUND = 5e-5


def _stage_output(seed=0):
    """A synthetic stage output [nseq, S, W]: rows of RMS 0.05 .. 3 plus outlier rows at ~30x (the stream's 'massive activations'), and the
    engine's copy of it with rounding noise at a tenth of the bound relative to each row."""
    g = torch.Generator().manual_seed(seed)
    nseq, S, W = 6, 37, 64
    ref = torch.randn(nseq, S, W, generator=g, dtype=torch.float64) * torch.logspace(math.log10(0.05), math.log10(3.0), S, dtype=torch.float64)[:, None]
    ref[:, 0] *= 30.0                                               # the CLS-like rows carry the tensor's maximum
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    got = ref + 0.1 * BOUND * rms * (2 * torch.rand(nseq, S, W, generator=g, dtype=torch.float64) - 1)
    return got.float().double(), ref, rms


def test_one_perturbed_row_is_flagged_where_the_global_metric_is_blind():
    got, ref, rms = _stage_output()
    assert worst_row(got, ref)[0] < 0.2 * BOUND                     # (fp32 storage adds 6e-8 relative: below the noise)
    s, t, c = 3, 11, 40
    got[s, t, c] += 4.0 * BOUND * float(rms[s, t])
    v, loc = worst_row(got, ref)
    assert loc == (s, t, c) and 3.5 * BOUND < v < 4.5 * BOUND
    e, _ = row_error(got, ref)
    assert int((e > BOUND).sum()) == 1
    assert global_error(got, ref) < BOUND                           # max |got - ref| / max |ref|: the same corruption passes
    log = StageLog("synthetic")
    log.check(4, "fc1", got, ref, BOUND)
    with pytest.raises(AssertionError, match=f"layer 4 fc1: .* at sequence {s}, token {t}, column {c}"):
        log.assert_ok()


def test_a_nan_row_is_never_within_bound():
    got, ref, _ = _stage_output(1)
    got[5, 36, 0] = float("nan")
    v, loc = worst_row(got, ref)
    assert v == math.inf and loc == (5, 36, 0)


def test_one_bad_tile_seam_row_among_many_sequences():
    """The bench shape's failure mode in miniature: the last row of one 256-row GEMM tile (a row in the middle of a packed sequence)
    off by 3x the bound, in a batch whose global maximum sits in other rows."""
    nseq, S, W = 8, 101, 32
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(nseq, S, W, generator=g, dtype=torch.float64)
    ref[:, 0] *= 30.0
    got = ref.clone()
    s, t = divmod(255, S)                                           # packed row 255 = sequence 2, token 53
    got[s, t] += 3.0 * BOUND * ref[s, t].pow(2).mean().sqrt()
    assert worst_row(got, ref)[1][:2] == (s, t) and global_error(got, ref) < BOUND


def _probe(mode, nseq, S, H, Md):
    """A StageProbe's geometry without an engine (its decoders are pure tensor code)."""
    pr = StageProbe.__new__(StageProbe)
    pr.mode, pr.H, pr.Md, pr.W = mode, H, Md, max(3 * H, Md)
    pr.S, pr.nseq = S, nseq
    pr.M_pad = (nseq * S + 255) // 256 * 256
    pr.rows_live = pr.M_pad + 128
    pr.planes = 2 if mode.endswith(("x3", "x2")) else 1
    pr.dtype = torch.float16 if mode.startswith("fp16") else torch.bfloat16
    return pr


@pytest.mark.parametrize("mode", ["fp16x3", "bf16"])
def test_decoders_follow_the_workspace_layout(mode):
    """lnbuf [planes][rows][H] and big [planes][rows][max(3H, M)] with rows of ld 3H (QKV) or M (MLP hidden); sequences at pitch S;
    planes_value = hi + lo."""
    nseq, S, H, Md = 3, 80, 8, 40                                   # nseq * S = 240: the batch pad is 16 rows + 128 slack
    pr = _probe(mode, nseq, S, H, Md)
    live = pr.rows_live

    def planes(v):                                                  # a value -> its hi (+ lo) planes in the mode's element type
        hi = v.to(pr.dtype)
        return torch.stack([hi, (v - hi.double()).to(pr.dtype)]) if pr.planes == 2 else hi[None]

    def val(k, width):                                              # exact in fp16 and bf16; encodes (row, column) per layout
        row, col = torch.arange(live)[:, None], torch.arange(width)
        return ((k * row + col // 8) % 31 + (col % 8) / 8).double()

    ln_val, qkv_val, fc1_val = val(1, H), val(2, 3 * H), val(3, Md)
    st = dict(x=torch.zeros(live, H), ln=planes(ln_val).reshape(pr.planes, -1))
    big = torch.zeros(pr.planes, live * pr.W, dtype=pr.dtype)
    big[:, :live * 3 * H] = planes(qkv_val).reshape(pr.planes, -1)
    st["big"] = big
    n = nseq * S
    assert torch.equal(pr.ln(st), ln_val[:n].view(nseq, S, H))
    assert torch.equal(pr.big(st, 3 * H), qkv_val[:n].view(nseq, S, 3 * H))
    big[:, :live * Md] = planes(fc1_val).reshape(pr.planes, -1)
    assert torch.equal(pr.big(st, Md), fc1_val[:n].view(nseq, S, Md))
    if pr.planes == 2:                                              # the lo plane is added: hi + lo carries more than one plane does
        st["ln"] = planes(ln_val + 2.0 ** -14).reshape(pr.planes, -1)
        assert torch.equal(pr.ln(st), (ln_val + 2.0 ** -14)[:n].view(nseq, S, H))
    # pad rows: nseq * S ... M_pad + 128, in x and in both row layouts of big
    assert pr.pad_rows_finite(st) == []
    st["x"][nseq * S + 3, 1] = float("inf")
    big[-1, (pr.M_pad + 100) * 3 * H + 2] = float("nan")
    assert pr.pad_rows_finite(st) == ["x", f"big (ld {3 * H})"]
    st["x"][nseq * S + 3, 1] = 0.0
    st["x"][nseq * S - 1, 1] = float("inf")                         # a sequence row, not a pad row: the stage comparison's business
    big[-1, (pr.M_pad + 100) * 3 * H + 2] = 0.0
    big[0, live * Md - 1] = float("nan")                            # the last slack row of the MLP-hidden layout
    assert pr.pad_rows_finite(st) == [f"big (ld {Md})"]
