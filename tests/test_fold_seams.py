"""The seam inputs of tests/fold_seams.py discriminate: for every length, layout, sequence and consumed token tests/test_gpu_fold_seams.py runs,
a fold that counts the wrong rows moves the sequence's fp64 output by at least 10 x (a dropped or admitted row, pass or chunk) or 5 x (a row or
chunk counted twice) the loosest bound the GPU file compares a kernel with, ATTN_TOL["bf16"] = 1.5e-2 of the sequence's max |ref|.  Runs on the
CPU in fp64 with the unrounded weights; this is the proof that the GPU tests can fail.  The smallest distances are printed (pytest -s).

Also here: the length list, the generator, the properties the argument rests on (row S - 1 holds at least a quarter of every head, logits stay
below 9.5, the chunked fp64 restatement of the fold agrees with the un-folded formula to 1e-12), and vtq_vl_cls_fold's declaration and the
refusals that need no device."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from tests import fold_seams as F

LOOSEST = 1.5e-2                                   # ATTN_TOL["bf16"] of tests/test_gpu_kernels.py (a GPU module: not imported here)
DROP_MIN, TWICE_MIN = 10 * LOOSEST, 5 * LOOSEST
HS = (768, 1024)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def bank(H):
    return F.Bank(F.parameters(H))


def gpu_cases():
    """(name, lengths, pitches, sequences to check, token of each): what the GPU file runs.  Uniform: three sequences of S, packed and padded,
    each with token 0 and S - 1; table-driven: all lengths in one packed call, as listed and reversed, token 0 for even j and S - 1 for odd."""
    for S in F.LENGTHS:
        for name, pitch in (("packed", S), ("padded", F.padded_pitch(S))):
            for token in sorted({0, S - 1}):
                yield f"uniform {name}", [S] * 3, [pitch] * 3, [token] * 3
    for name, lengths in (("as listed", F.LENGTHS), ("reversed", F.LENGTHS[::-1])):
        yield f"table {name}", list(lengths), None, [0 if j % 2 == 0 else S - 1 for j, S in enumerate(lengths)]


def exempt(S, w):
    # one key counted twice is the same softmax; a sequence of one chunk has no chunk to lose or to repeat apart from ALL of it (no rows:
    # NaN, an infinite distance) or all of it twice (the same softmax again)
    return (w == "count_last_twice" and S == 1) or (w in ("drop_last_chunk", "last_chunk_twice") and S <= F.CHUNK)


def test_lengths_are_the_seams_of_the_fold():
    assert F.LENGTHS == [1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 319, 320, 321, 511, 512, 513,
                         575, 576, 577]
    assert F.CHUNK == 64 and F.SUB == 32 and max(F.LENGTHS) <= F.BANK_ROWS
    for g in (F.SUB, F.CHUNK):
        assert {g - 1, 0, 1} <= {S % g for S in F.LENGTHS if S >= g - 1}
    chunks = {(S + F.CHUNK - 1) // F.CHUNK for S in F.LENGTHS}
    assert {1, 2, 3, 4, 5, 6, 8, 9, 10} <= chunks          # both sides of the combine kernel's batches of 4 and of 8


def test_the_generator_is_what_the_docstring_says():
    par = F.parameters(768)
    b = bank(768)
    N = b.N
    assert torch.equal(b.x[:N], par["noise"]) and torch.equal(b.x[N:], par["noise"] + par["d"])
    assert torch.equal(par["W"][0], par["W"][768]) and torch.equal(par["W"][64 * 5], par["d"] / 768 ** 0.5)
    lengths, pitches = [5, 33, 1], [F.padded_pitch(5), F.padded_pitch(33), F.padded_pitch(1)]
    assert pitches == [96, 128, 96]
    ident, starts = F.layout(lengths, pitches)
    assert starts == [0, 96, 224] and ident.shape[0] == 320 + F.SLACK
    spiked = (ident >= N).nonzero().flatten().tolist()
    assert spiked == sorted({0, *range(4, 96), 96, *range(128, 224), *range(224, 320 + F.SLACK)})
    assert (ident[:5] % N).tolist() == [0, 1, 2, 3, 4] and (ident[96:129] % N).tolist() == list(range(F.BANK_ROWS, F.BANK_ROWS + 33))
    fill = F.filler_rows(lengths, pitches)
    assert fill.nonzero().flatten().tolist() == sorted({*range(5, 96), *range(129, 224), *range(225, 320 + F.SLACK)})
    assert bool((ident[fill] % N >= 3 * F.BANK_ROWS).all()) and not bool((ident[~fill] % N >= 3 * F.BANK_ROWS).any())
    packed, pstarts = F.layout(lengths)
    for (r0, p0, S) in zip(starts, pstarts, lengths):                          # a sequence has the same rows at every pitch
        assert torch.equal(ident[r0:r0 + S], packed[p0:p0 + S])
    # the bank's K and V are the row-wise projections of the rows a kernel is handed
    x = b.x[ident[:40]]
    ln = F.layer_norm64(x, b.lw, b.lb)
    assert torch.equal(ln, b.ln[ident[:40]])
    assert float((ln @ b.W[768:1536].t() + b.b[768:1536] - b.k[ident[:40]]).abs().max()) < 1e-12
    # u lies along d: per head, the part of W_k,h^T q_h off d is a few per cent of it
    q = F.query(b, ident, 0, 5, 0, False).double().view(12, 64)
    u = torch.einsum("hd,hdk->hk", q, b.W[768:1536].view(12, 64, 768))
    dh = par["d"].double() / par["d"].double().norm()
    off = (u - (u @ dh)[:, None] * dh).norm(dim=-1) / u.norm(dim=-1)
    assert 0.002 < float(off.min()) and float(off.max()) < 0.05, off


@pytest.mark.parametrize("H", HS)
def test_row_s_minus_1_dominates_logits_stay_moderate_and_the_fold_is_the_unfolded_formula(H):
    b = bank(H)
    low, high, top, gap = 1.0, 0.0, 0.0, 0.0
    for name, lengths, pitches, tokens in gpu_cases():
        ident, starts = F.layout(lengths, pitches)
        for j, (r0, S, token) in enumerate(zip(starts, lengths, tokens)):
            for q_log2 in (False, True):
                q = F.query(b, ident, r0, S, token, q_log2)
                ref, p, _ = F.attention_ref(b, ident, r0, S, q, q_log2)
                fold, logit = F.folded_ref(b, ident, r0, S, q, q_log2)
                gap = max(gap, F.distance(fold, ref, ref.abs().max()))
                top = max(top, logit)
                if S > 1:
                    low, high = min(low, float(p[:, S - 1].min())), max(high, float(p[:, S - 1].max()))
    print(f"H={H}: row S - 1 holds {low:.3f} .. {high:.3f} of a head, largest |logit| {top:.2f}, folded vs un-folded fp64 {gap:.1e}")
    assert low >= 0.25 and top < 9.5 and gap < 1e-12


@pytest.mark.parametrize("H", HS)
def test_every_wrong_row_mask_moves_every_sequence_by_many_bounds(H):
    b = bank(H)
    smallest = {w: (float("inf"), None) for w in F.WRONG}
    misses = []
    for name, lengths, pitches, tokens in gpu_cases():
        ident, starts = F.layout(lengths, pitches)
        for j, (r0, S, token) in enumerate(zip(starts, lengths, tokens)):
            for q_log2 in (False, True):
                q = F.query(b, ident, r0, S, token, q_log2)
                ref = F.attention_ref(b, ident, r0, S, q, q_log2)[0]
                for w in F.WRONG:
                    if exempt(S, w):
                        continue
                    dist = F.distance(F.attention_ref(b, ident, r0, S, q, q_log2, w)[0], ref, ref.abs().max())
                    if dist < smallest[w][0]:
                        smallest[w] = (dist, (name, S, j, token, "log2" if q_log2 else "natural"))
                    if not dist >= (TWICE_MIN if w.endswith("twice") else DROP_MIN):
                        misses.append((w, name, S, j, token, q_log2, dist))
    for w in F.WRONG:
        print(f"H={H} smallest distance of {w}: {smallest[w][0]:.3g} of max |ref| at (case, S, sequence, token, units) = {smallest[w][1]}   "
              f"(floor {TWICE_MIN if w.endswith('twice') else DROP_MIN:g})")
    assert not misses, misses


def test_wrong_variants_count_the_rows_their_names_say():
    assert F.rows_of(65, "drop_last") == list(range(64)) and F.rows_of(65, "admit_next") == list(range(66))
    assert F.rows_of(65, "drop_last_sub") == F.rows_of(65, "drop_last_chunk") == list(range(64))
    assert F.rows_of(64, "drop_last_sub") == list(range(32)) and F.rows_of(64, "drop_last_chunk") == [] == F.rows_of(1, "drop_last")
    assert F.rows_of(97, "drop_last_sub") == list(range(96)) and F.rows_of(97, "drop_last_chunk") == list(range(64))
    assert F.rows_of(3, "count_last_twice") == [0, 1, 2, 2]
    assert F.rows_of(130, "last_chunk_twice") == list(range(130)) + [128, 129] and F.rows_of(128, "last_chunk_twice") == list(range(128)) + list(range(64, 128))


# ---- vtq_vl_cls_fold without a GPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vtamiq_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_lib_binds_the_table_driven_fold(lib):
    from vtamiq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    assert re.search(r"^int\s+vtq_vl_cls_fold\(", hdr, re.M)
    assert lib.vtq_vl_cls_fold.argtypes == _lib.SIGNATURES["vtq_vl_cls_fold"][1]
    uniform, table = _lib.SIGNATURES["vtq_k_cls_fold"][1], _lib.SIGNATURES["vtq_vl_cls_fold"][1]
    assert len(table) == len(uniform) - 1                  # seq_len in place of S and seq_stride
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION == lib.vtq_abi_version()
    assert lib.vtq_k_cls_fold_chunk_rows() == F.CHUNK


def test_table_driven_fold_refuses_bad_arguments_without_touching_a_device(lib):
    fake = C.c_void_p(0x1000)                      # never dereferenced: every call below is refused on an argument checked before any device call
    one, zero = (C.c_int32 * 1)(8), (C.c_int32 * 2)(8, 0)
    err = lambda: lib.vtq_last_error()

    def call(q=fake, x=fake, nseq=1, seq_len=one, H=768, num=19, q_log2=0, ctx=fake):
        return lib.vtq_vl_cls_fold(q, fake, 3 * H * H, fake, x, fake, fake, nseq, seq_len, H, num, q_log2, fake, fake, fake, 64 * (H // 64) * H, ctx, None)
    for what, kw, word in (("NULL q", dict(q=None), b"null"), ("NULL x", dict(x=None), b"null"), ("NULL seq_len", dict(seq_len=None), b"null"),
                           ("NULL ctx", dict(ctx=None), b"null"), ("nseq = 0", dict(nseq=0), b"nseq=0"),
                           ("a length of 0", dict(nseq=2, seq_len=zero), b"sequence 1 has length 0"), ("H = 512", dict(H=512), b"H=512"),
                           ("unknown format", dict(num=99), b"format"), ("q_log2 on a 1-term format", dict(num=17, q_log2=1), b"q_log2")):
        assert call(**kw) != 0, what + ": accepted"
        assert b"vtq_vl_cls_fold" in err() and word in err(), (what, err())
