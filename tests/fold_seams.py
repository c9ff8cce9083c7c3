"""Inputs and fp64 references for the folded single-query attention of the CLS tail at the seam lengths (no GPU code: importable anywhere).

cls_key_fold_kernel, cls_fold_attention_kernel and cls_fold_combine_kernel (csrc/cls_tail.hip) decide by a sequence's length S which fp32
rows count as keys: the row loads and the LayerNorm step (`srow < S`, `live`), the score mask (`s0 + row >= S`), the number of 32-row passes
of the last chunk, the early return of the table-driven form and the chunk count of the combine kernel, whose batched loads clamp an index
past the end to the last chunk.  On Gaussian rows one key holds about 1/S of a head's probability and a row of zeros normalises to ln_b, so a
mask off by one row stays far below the bounds of the single-plane formats.  Here row S - 1 and every row a kernel could reach but must not
count hold a third to a half of each head's probability (tests/test_fold_seams.py proves on the CPU that every wrong mask below moves a
sequence's output by many bounds; tests/test_gpu_fold_seams.py runs the kernels).

What is harder than in tests/attention_seams.py: a row's value, W_v ln_s, is tied to the same ln_s = LayerNorm(x_s) that sets its score, so the
dominant rows cannot be given a key and a value separately.  Construction:
    rows      ordinary x_s = N(0, 1); spike x_s = d + N(0, 1) for ONE fixed direction d = N(0, 1)^H: ln_spike is about (d + n_s) / sqrt(2), so
              spikes agree along d and differ in their own noise -- their values W_v ln_s differ by about as much as the common part
    W_k, W_q  row 64 h of each is d / sqrt(H); the other rows of W_k are N(0, 1) / sqrt(H), those of W_q and b_q small (Q_NOISE): the query of a
              spike token is about (d . ln) / sqrt(H) e_0 per head, and u_h = W_k,h^T q_h lies along d plus about 2 % of per-head noise
    q         the fp64 query projection of the consumed token (row 0 or S - 1, both spikes), times ONE scale per sequence: the one that puts
              the logit of row S - 1, less the part every row shares (ln_b and b_k), at ln S + MARGIN on average over the heads.  q is an
              input of the entry, so the scale needs no weight of its own
    LayerNorm lw = 1 + 0.2 N, lb = 0.1 N;    W_v = N / sqrt(H), b = 0.3 N (b_q: Q_NOISE N)
    spikes    row 0 and row S - 1 of every sequence; the gap rows [S, pitch) of a padded layout; the 64 SLACK rows behind the last sequence
              (packed: the row behind S - 1 is the next sequence's row 0, a spike already)
A spike weighs about S e^MARGIN, four times the ordinary rows of its sequence together: row S - 1 holds 0.3 .. 0.6 of every head (1 at S = 1)
and logits stay below 9.  MARGIN and the noise scales are set by the CPU conditions alone.

Rows come from a bank: NOISE_COPIES x BANK_ROWS seeded N(0, 1) rows, each in an ordinary and a spiked version.  Sequence j of a case is the
first S rows of copy j % 3 (so a sequence has the same rows at every pitch and in every call), the filler rows are spiked rows of copy 3.  A
layout is the (rows,) index tensor into the bank; K and V of the un-folded reference are row-wise functions of x, so they are computed
once per bank row (Bank) and gathered.

References: the UN-folded fp64 formula of tests/test_gpu_cls_fold.py (LayerNorm, K and V of every row, softmax of q . k, P V; exp2 when q
arrives in log2 units) over a list of rows; the wrong variants are other lists (rows_of).  folded_ref restates the fold itself in fp64 --
partials (m, l, z) per CHUNK rows, combined in chunk order, then the value projection -- and must agree with the un-folded one."""
import math

import torch

CHUNK = 64                      # vtq_k_cls_fold_chunk_rows(); the GPU file asserts it
SUB = 32                        # rows of one LDS pass of cls_fold_attention_kernel
SLACK = 64                      # spiked rows behind the last sequence
BANK_ROWS = 640
NOISE_COPIES = 4                # three for sequences, one for gap and slack rows
MARGIN = 1.5
Q_NOISE = 0.04
WRONG = ("drop_last", "admit_next", "drop_last_sub", "drop_last_chunk", "count_last_twice", "last_chunk_twice")
LOG2_SCALE = 0.125 * math.log2(math.e)          # what the 3-term formats' query projection folds into q


def seam_lengths(c=CHUNK):
    """One below, at and above every multiple of c / 2 up to 2 c (the 32-row pass and the chunk) and of c at the chunk counts 3|4, 4|5, 5|6, 8|9
    and 9|10 (the combine kernel loads chunks in batches of 4 and of 8), the smallest lengths, and one length off every granule."""
    at = [k * c // 2 for k in (1, 2, 3, 4)] + [n * c for n in (3, 4, 5, 8, 9)]
    return sorted({1, 2, 3, 5 * c - 20} | {a + e for a in at for e in (-1, 0, 1)})


LENGTHS = seam_lengths()


def ceil_to(a, b):
    return (a + b - 1) // b * b


def padded_pitch(S):
    """Rows from one sequence to the next in the padded layout: S rounded up to 32, and a whole chunk of gap rows."""
    return ceil_to(S, SUB) + CHUNK


# ---- parameters and the row bank -------------------------------------------------------------------------------------------------------------
def parameters(H, seed=2203):
    """fp32 on the CPU: d (H), lw, lb (H), W (3H, H) = query | key | value, b (3H)."""
    g = torch.Generator(device="cpu").manual_seed(seed + H)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = rn(H)
    lw, lb = 1.0 + 0.2 * rn(H), 0.1 * rn(H)
    Wq, Wk, Wv = Q_NOISE * rn(H, H) / math.sqrt(H), rn(H, H) / math.sqrt(H), rn(H, H) / math.sqrt(H)
    Wq[0::64] = d / math.sqrt(H)
    Wk[0::64] = d / math.sqrt(H)
    b = torch.cat([Q_NOISE * rn(H), 0.3 * rn(H), 0.3 * rn(H)])
    noise = rn(NOISE_COPIES * BANK_ROWS, H)
    return {"H": H, "d": d, "lw": lw, "lb": lb, "W": torch.cat([Wq, Wk, Wv]), "b": b, "noise": noise}


class Bank:
    """Every distinct row of every case and what the un-folded formula needs of it, in fp64 on W's device: x (fp32, as a kernel reads it),
    ln = LayerNorm(x), k and v.  Row i < N is noise row i, row N + i its spiked version.  W: the (3H, H) weights AS THE KERNELS READ THEM
    (fp64; the values of the operand planes on the GPU, the fp32 draw on the CPU)."""

    def __init__(self, par, W=None):
        W = par["W"].double() if W is None else W
        dev = W.device
        H = self.H = par["H"]
        self.nh, self.N = H // 64, NOISE_COPIES * BANK_ROWS
        self.W, self.b = W, par["b"].to(dev).double()
        self.lw, self.lb = par["lw"].to(dev).double(), par["lb"].to(dev).double()
        noise = par["noise"].to(dev)
        self.x = torch.cat([noise, noise + par["d"].to(dev)]).contiguous()
        self.ln = layer_norm64(self.x, self.lw, self.lb)
        self.k = self.ln @ W[H:2 * H].t() + self.b[H:2 * H]
        self.v = self.ln @ W[2 * H:].t() + self.b[2 * H:]


def layer_norm64(x, lw, lb):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * lw + lb


def layout(lengths, pitches=None):
    """(bank row of every buffer row (rows + SLACK,), first row of every sequence): sequence j = rows [0, S) of noise copy j % 3, rows 0 and S - 1
    spiked; every other row a spiked row of copy 3."""
    pitches = list(lengths) if pitches is None else list(pitches)
    assert len(pitches) == len(lengths) and all(p >= s >= 1 and s <= BANK_ROWS for s, p in zip(lengths, pitches))
    N = NOISE_COPIES * BANK_ROWS
    rows = sum(pitches)
    ident = N + 3 * BANK_ROWS + torch.arange(rows + SLACK) % BANK_ROWS
    starts, r0 = [], 0
    for j, (S, p) in enumerate(zip(lengths, pitches)):
        ident[r0:r0 + S] = (j % 3) * BANK_ROWS + torch.arange(S)
        ident[r0] += N
        if S > 1:
            ident[r0 + S - 1] += N
        starts.append(r0)
        r0 += p
    return ident, starts


def filler_rows(lengths, pitches=None):
    """bool (rows + SLACK,): the gap and slack rows, which belong to no sequence."""
    ident, starts = layout(lengths, pitches)
    f = torch.ones(ident.shape[0], dtype=torch.bool)
    for r0, S in zip(starts, lengths):
        f[r0:r0 + S] = False
    return f


# ---- the query -------------------------------------------------------------------------------------------------------------------------------
def query(bank, ident, r0, S, token, q_log2):
    """fp32 (H,): the query projection of row `token` of the sequence at r0, scaled so that row S - 1 scores ln S + MARGIN above the part all
    rows share, on average over the heads; in log2 units when q_log2 (the entry then applies neither 1/8 nor log2 e)."""
    H, nh = bank.H, bank.nh
    q = (bank.ln[int(ident[r0 + token])] @ bank.W[:H].t() + bank.b[:H]).view(nh, 64)
    last = int(ident[r0 + S - 1])
    shared = bank.lb @ bank.W[H:2 * H].t() + bank.b[H:2 * H]
    lead = 0.125 * (q * (bank.k[last] - shared).view(nh, 64)).sum(-1)
    q = q * ((math.log(S) + MARGIN) / lead.mean())
    return (q.reshape(H) * (LOG2_SCALE if q_log2 else 1.0)).float().contiguous()


# ---- fp64 references -------------------------------------------------------------------------------------------------------------------------
def rows_of(S, variant="true", c=CHUNK):
    """Rows of a sequence (relative to its first) that a kernel with this mask would count; admit_next takes row S of the buffer."""
    if variant == "true":
        return list(range(S))
    if variant == "drop_last":
        return list(range(S - 1))
    if variant == "admit_next":
        return list(range(S + 1))
    if variant == "drop_last_sub":                       # the last 32-row pass is not run
        return list(range((S - 1) // SUB * SUB))
    if variant == "drop_last_chunk":                     # the last chunk's partial is not combined
        return list(range((S - 1) // c * c))
    if variant == "count_last_twice":
        return list(range(S)) + [S - 1]
    if variant == "last_chunk_twice":                    # the combine kernel's clamped re-read of the last chunk is used
        return list(range(S)) + list(range((S - 1) // c * c, S))
    raise KeyError(variant)


def attention_ref(bank, ident, r0, S, q, q_log2, variant="true"):
    """Un-folded: ((H,) ctx, (nh, keys) probabilities, (nh, keys) scores) over the variant's rows; no row at all: NaN."""
    nh = bank.nh
    rel = rows_of(S, variant)
    if not rel:
        nan = torch.full((bank.H,), float("nan"), dtype=torch.float64, device=bank.k.device)
        return nan, nan[:0].view(nh, 0), nan[:0].view(nh, 0)
    idx = ident[r0 + torch.tensor(rel)].to(bank.k.device)
    k, v = bank.k[idx].view(-1, nh, 64), bank.v[idx].view(-1, nh, 64)
    s = torch.einsum("hd,shd->hs", q.double().view(nh, 64), k)
    if not q_log2:
        s = s * 0.125
    e = s - s.amax(-1, keepdim=True)
    p = torch.exp2(e) if q_log2 else torch.exp(e)
    p = p / p.sum(-1, keepdim=True)
    return torch.einsum("hs,shd->hd", p, v).reshape(bank.H), p, s


def folded_ref(bank, ident, r0, S, q, q_log2, c=CHUNK):
    """The fold restated in fp64: u_h = W_k,h^T q_h; per chunk of c rows (m, l, z) of the scores u_h . ln_s; the chunks combined in ascending
    order with a running maximum; ctx_h = W_v,h (z_h / l_h) + b_v,h.  Returns (ctx (H,), the largest score a kernel forms, in natural units)."""
    H, nh = bank.H, bank.nh
    ex = torch.exp2 if q_log2 else torch.exp
    u = torch.einsum("hd,hdk->hk", q.double().view(nh, 64), bank.W[H:2 * H].view(nh, 64, H)) * (1.0 if q_log2 else 0.125)
    ln = bank.ln[ident[r0:r0 + S].to(bank.ln.device)]
    M = torch.full((nh,), -float("inf"), dtype=torch.float64, device=ln.device)
    L, Z, top = torch.zeros_like(M), torch.zeros(nh, H, dtype=torch.float64, device=ln.device), -float("inf")
    for c0 in range(0, S, c):
        rows = ln[c0:c0 + c]
        sc = rows @ u.t()                                   # (rows, nh)
        m = sc.amax(0)
        w = ex(sc - m)
        l, z = w.sum(0), w.t() @ rows
        Mn = torch.maximum(M, m)
        a, bb = ex(M - Mn), ex(m - Mn)
        L, Z, M = a * L + bb * l, a[:, None] * Z + bb[:, None] * z, Mn
        top = max(top, float(sc.abs().max()))
    zbar = Z / L[:, None]
    ctx = torch.einsum("hdk,hk->hd", bank.W[2 * H:].view(nh, 64, H), zbar) + bank.b[2 * H:].view(nh, 64)
    return ctx.reshape(H), top / (math.log2(math.e) if q_log2 else 1.0)


def distance(a, b, scale):
    """max |a - b| / scale; a NaN on either side is an infinite distance."""
    d = (a - b).abs().max()
    return float("inf") if bool(torch.isnan(d)) else float(d / scale)
