"""The folded single-query attention of the CLS tail (csrc/cls_tail.hip: cls_key_fold_kernel, cls_fold_attention_kernel, cls_fold_combine_kernel
and the value projection) against fp64 at every seam length, on inputs where the boundary rows dominate (tests/fold_seams.py: row S - 1 and
every row a kernel could reach but must not count hold a third to a half of each head's probability; tests/test_fold_seams.py shows on the CPU
that a fold which drops or admits a row, a 32-row pass or a chunk moves every sequence by at least 10 x the loosest bound used here, and one
that counts the last row or the last chunk twice by at least 5 x).

Entries: vtq_k_cls_fold (three sequences per length, so cls_key_fold_kernel has a partial 4-row group; packed pitch and seq_stride =
(ceil32(S) + 64) H; consumed token 0 and S - 1) and vtq_vl_cls_fold (all 31 lengths in ONE packed call, as listed and reversed); formats
fp16x3, bf16x3, fp16, bf16 at H = 768 and fp16x3, bf16 at H = 1024 (the other template instance: 16 heads, no dead head column).  One test per
(entry, format, H) loops over the lengths and collects (S, sequence, where, error) of every miss, so one run names every bad length.

Besides the comparison with fp64, per length: the packed and the padded call give the same bits per sequence, and so does a third call whose
gap and slack rows are NaN (a sequence's result depends on its own rows and S only); every sequence of the table-driven call has the bits of
vtq_k_cls_fold(nseq = 1, S = its length) on its rows; u, part and ctx are pre-filled with NaN and 64 spare floats behind each stay NaN, as do
the chunk slots of `part` behind a sequence's own chunks.

The bound is ATTN_TOL[format] (tests/test_gpu_kernels.py) of the sequence's max |ref|: the project's bound for the attention output in that
format.  The fold forms the same quantity with less rounding (K, V and P stay fp32; only zbar and W_v go through operand planes).
Measured on the MI355X, worst over every length, layout, token and sequence (the `measured` lines; per length: profiles/r19_fold_seams.txt):
                         fp16x3     bf16x3     fp16       bf16        fp16x3 H=1024   bf16 H=1024
    vtq_k_cls_fold       7.58e-7    6.22e-6    3.06e-4    2.48e-3     8.71e-7         2.09e-3      bound ATTN_TOL    1e-5  2e-4  3e-3  1.5e-2
    vtq_vl_cls_fold      7.58e-7    4.96e-6    2.83e-4    2.31e-3     8.65e-7         2.09e-3
No bound is relaxed: the fold stays 6 to 30 times inside the attention kernels' bounds.  The errors are at one level from S = 1 to 577 (within a
factor 4 per format), with no step at a 32-row pass, a chunk or a batch of the combine kernel's loads.  No mask was found wrong.
"""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import fold_seams as F
from tests.gpu_util import FORMATS, elt_dtype, num_code, planes_value, stream, to_planes
from tests.test_gpu_kernels import ATTN_TOL
from vtamiq_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NSEQ = 3
SPARE = 64
INF = float("inf")
NAN = float("nan")
CASES = [("fp16x3", 768), ("bf16x3", 768), ("fp16", 768), ("bf16", 768), ("fp16x3", 1024), ("bf16", 1024)]
ORDERS = {"as listed": F.LENGTHS, "reversed": F.LENGTHS[::-1]}
_table = {}                                      # (entry, format, H, S) -> (worst error, where)


@pytest.fixture(scope="module", autouse=True)
def seam_table():
    """With VTQ_FOLD_SEAM_TABLE=<path> in the environment the per-length table of this run is written there (profiles/r19_fold_seams.txt is
    one), behind the '#' lines an existing file begins with."""
    yield
    path = os.environ.get("VTQ_FOLD_SEAM_TABLE")
    if path and _table:
        header = []
        if os.path.exists(path):
            with open(path) as f:
                for line in f:
                    if not line.startswith("#"):
                        break
                    header.append(line)
        with open(path, "w") as f:
            f.writelines(header)
            f.write("entry             format   H      S     worst error   where\n")
            order = [c[0] for c in CASES]
            for (entry, fmt, H, S), (err, where) in sorted(_table.items(), key=lambda kv: (kv[0][0], kv[0][2], order.index(kv[0][1]), kv[0][3])):
                f.write(f"{entry:<17} {fmt:<8} {H:<6} {S:<5} {err:<13.3e} {where}\n")


def note(entry, fmt, H, S, err, where):
    if (entry, fmt, H, S) not in _table or not err <= _table[(entry, fmt, H, S)][0]:
        _table[(entry, fmt, H, S)] = (err, where)


def measured(entry, fmt, H, bound):
    rows = [(v[0], S, v[1]) for (e, f, h, S), v in _table.items() if (e, f, h) == (entry, fmt, H)]
    err, S, where = max(rows)
    print(f"measured {entry} {fmt} H={H}: {err:.2e} at S = {S}, {where} (bound {bound:g}, {len(rows)} lengths)")


class Setup:
    """The parameters of one (format, H) on the device: the weight planes, the fp32 vectors the entries read, and the bank of rows with its
    fp64 K and V from the weights as the planes hold them."""

    def __init__(self, fmt, H):
        par = F.parameters(H)
        self.fmt, self.H, self.nh = fmt, H, H // 64
        self.q_log2 = FORMATS[fmt][1] == 3
        self.apl = 2 if FORMATS[fmt][1] > 1 else 1
        self.Wp = to_planes(par["W"].to(DEV), fmt, "w")
        self.lw, self.lb, self.b = par["lw"].to(DEV), par["lb"].to(DEV), par["b"].to(DEV)
        self.bank = F.Bank(par, planes_value(self.Wp))

    def rows(self, ident):
        return self.bank.x[ident.to(DEV)].contiguous()

    def queries(self, ident, starts, lengths, tokens):
        return torch.stack([F.query(self.bank, ident, r0, S, t, self.q_log2) for r0, S, t in zip(starts, lengths, tokens)]).contiguous()

    def workspace(self, nseq, chunks):
        H, nh = self.H, self.nh
        n = {"u": nseq * nh * H, "part": nseq * chunks * nh * (H + 2), "ctx": nseq * H}
        w = {k: torch.full((v + SPARE,), NAN, device=DEV) for k, v in n.items()}
        w["z"] = torch.zeros((self.apl, 64, nh * H), dtype=elt_dtype(self.fmt), device=DEV)
        return n, w

    def spares_kept(self, n, w):
        return all(bool(torch.isnan(w[k][n[k]:]).all()) for k in n)

    def uniform(self, x, stride_rows, q, nseq, S):
        """(ctx (nseq, H), the spares stayed NaN)"""
        lib, H = _lib.load(), self.H
        assert q.shape == (nseq, H) and x.shape[0] >= (nseq - 1) * stride_rows + S and nseq <= 64
        n, w = self.workspace(nseq, (S + F.CHUNK - 1) // F.CHUNK)
        _lib.check(lib.vtq_k_cls_fold(q.data_ptr(), self.Wp.data_ptr(), 3 * H * H, self.b.data_ptr(), x.data_ptr(), stride_rows * H, self.lw.data_ptr(),
                                      self.lb.data_ptr(), nseq, S, H, num_code(self.fmt), int(self.q_log2), w["u"].data_ptr(), w["part"].data_ptr(),
                                      w["z"].data_ptr(), 64 * self.nh * H, w["ctx"].data_ptr(), stream()))
        torch.cuda.synchronize()
        return w["ctx"][:n["ctx"]].view(nseq, H), self.spares_kept(n, w)

    def table(self, x, q, lengths):
        """(ctx (nseq, H), the spares and the chunk slots behind each sequence's own stayed NaN and its own are written)"""
        lib, H, nseq = _lib.load(), self.H, len(lengths)
        assert q.shape == (nseq, H) and x.shape[0] >= sum(lengths) and nseq <= 64
        cmax = (max(lengths) + F.CHUNK - 1) // F.CHUNK
        n, w = self.workspace(nseq, cmax)
        arr = (C.c_int32 * nseq)(*lengths)
        _lib.check(lib.vtq_vl_cls_fold(q.data_ptr(), self.Wp.data_ptr(), 3 * H * H, self.b.data_ptr(), x.data_ptr(), self.lw.data_ptr(), self.lb.data_ptr(),
                                       nseq, arr, H, num_code(self.fmt), int(self.q_log2), w["u"].data_ptr(), w["part"].data_ptr(), w["z"].data_ptr(),
                                       64 * self.nh * H, w["ctx"].data_ptr(), stream()))
        torch.cuda.synchronize()
        kept = self.spares_kept(n, w)
        slots = torch.isnan(w["part"][:n["part"]].view(nseq, cmax, -1))
        for j, S in enumerate(lengths):
            own = (S + F.CHUNK - 1) // F.CHUNK
            kept = kept and bool(slots[j, own:].all()) and not bool(slots[j, :own].any())
        return w["ctx"][:n["ctx"]].view(nseq, H), kept


@functools.lru_cache(maxsize=2)
def setup(fmt, H):
    return Setup(fmt, H)


def bits(t):
    return t.contiguous().view(torch.int32)


def error(got, ref):
    return F.distance(got.double(), ref, ref.abs().max())


def test_the_library_folds_in_chunks_of_the_length_list():
    assert _lib.load().vtq_k_cls_fold_chunk_rows() == F.CHUNK and F.LENGTHS == F.seam_lengths(F.CHUNK)


# ---- vtq_k_cls_fold --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,H", CASES)
def test_uniform_fold_against_fp64_at_every_seam(fmt, H):
    su = setup(fmt, H)
    bound, misses = ATTN_TOL[fmt], []
    for S in F.LENGTHS:
        pitch = F.padded_pitch(S)
        ident, starts = F.layout([S] * NSEQ)
        ident_g, starts_g = F.layout([S] * NSEQ, [pitch] * NSEQ)
        xp, xg = su.rows(ident), su.rows(ident_g)
        xn = xg.clone()
        xn[F.filler_rows([S] * NSEQ, [pitch] * NSEQ).to(DEV)] = NAN
        for token in sorted({0, S - 1}):
            q = su.queries(ident, starts, [S] * NSEQ, [token] * NSEQ)
            got, kept = su.uniform(xp, S, q, NSEQ, S)
            runs = {"packed": (got, kept), "padded": su.uniform(xg, pitch, q, NSEQ, S), "padded, gap and slack rows NaN": su.uniform(xn, pitch, q, NSEQ, S)}
            for j, r0 in enumerate(starts):
                ref = F.attention_ref(su.bank, ident, r0, S, q[j], su.q_log2)[0]
                e = error(got[j], ref)
                where = f"token {token} sequence {j}"
                note("vtq_k_cls_fold", fmt, H, S, e, where)
                if not e < bound:
                    misses.append((S, j, where, e))
                for name, (other, _) in runs.items():
                    if not (torch.equal(bits(other[j]), bits(got[j])) and bool(torch.isfinite(other[j]).all())):
                        misses.append((S, j, f"{where}: the {name} call differs from the packed one or is not finite", INF))
            for name, (_, kept) in runs.items():
                if not kept:
                    misses.append((S, NSEQ, f"token {token}, {name}: an element past u, part or ctx was written", INF))
    measured("vtq_k_cls_fold", fmt, H, bound)
    assert not misses, misses


# ---- vtq_vl_cls_fold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,H", CASES)
def test_table_driven_fold_against_fp64_and_the_uniform_entry_at_every_seam(fmt, H):
    su = setup(fmt, H)
    bound, misses = ATTN_TOL[fmt], []
    for order, lengths in ORDERS.items():
        lengths = list(lengths)
        ident, starts = F.layout(lengths)
        x = su.rows(ident)
        tokens = [0 if j % 2 == 0 else S - 1 for j, S in enumerate(lengths)]
        q = su.queries(ident, starts, lengths, tokens)
        got, kept = su.table(x, q, lengths)
        if not kept:
            misses.append((0, len(lengths), f"{order}: an element past u, part or ctx, or a chunk slot that is not the sequence's own, was written", INF))
        for j, (r0, S) in enumerate(zip(starts, lengths)):
            ref = F.attention_ref(su.bank, ident, r0, S, q[j], su.q_log2)[0]
            e = error(got[j], ref)
            where = f"{order}, sequence {j} at row {r0}, token {tokens[j]}"
            note("vtq_vl_cls_fold", fmt, H, S, e, where)
            if not e < bound:
                misses.append((S, j, where, e))
            alone, _ = su.uniform(x[r0:], S, q[j:j + 1], 1, S)
            if not torch.equal(bits(alone[0]), bits(got[j])):
                misses.append((S, j, f"{where}: not the bits of vtq_k_cls_fold(nseq = 1, S = {S}) on its rows", INF))
    measured("vtq_vl_cls_fold", fmt, H, bound)
    assert not misses, misses


# ---- the comparison compares something -------------------------------------------------------------------------------------------------------
def test_the_kernel_is_ten_bounds_away_from_a_fold_that_drops_or_admits_a_row():
    """S = 129 (one row past two chunks) and S = 321 (one past five: the second batch of the combine kernel's loads), bf16, the loosest bound:
    against the fp64 answer without row S - 1, and against the one with row S as well, the same comparison as above misses its bound at
    least tenfold in every sequence.  (Against the true answer it holds: the tests above.)"""
    su = setup("bf16", 768)
    for S in (129, 321):
        ident, starts = F.layout([S] * NSEQ)
        q = su.queries(ident, starts, [S] * NSEQ, [S - 1] * NSEQ)
        got, _ = su.uniform(su.rows(ident), S, q, NSEQ, S)
        for j, r0 in enumerate(starts):
            true = F.attention_ref(su.bank, ident, r0, S, q[j], su.q_log2)[0]
            for w in ("drop_last", "admit_next"):
                wrong = F.attention_ref(su.bank, ident, r0, S, q[j], su.q_log2, w)[0]
                err = F.distance(got[j].double(), wrong, true.abs().max())
                assert err >= 10 * ATTN_TOL["bf16"], (S, j, w, err)
