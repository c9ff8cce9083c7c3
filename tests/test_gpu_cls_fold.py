"""The folded single-query attention of the CLS-only last layer (csrc/cls_tail.hip: cls_key_fold_kernel, cls_fold_attention_kernel,
cls_fold_combine_kernel, and the value projection on skinny_linear_kernel with a column offset per head), through vtq_k_cls_fold.

With one query per (sequence, head) the engine never forms K or V of the last layer:
    score[s,h] = (W_k,h^T q_h) . ln_s + const(h),        ctx_h = W_v,h (sum_s p[s,h] ln_s) + b_v,h,        ln_s = LayerNorm(x_s)
The reference here is the UN-folded formula in fp64 (LayerNorm, K and V of every row, softmax, P V) from the same x and the weights as
the kernels read them (hi + lo planes).  The accuracy bound is not a constant: the same error is measured for the full-layer kernels
(vtq_k_layernorm -> vtq_k_gemm (QKV) -> vtq_k_attention, row of the consumed token) on the same inputs, and the fold may have twice that
(both are rounding-level and differ in summation order only).  Error = max |got - ref| / rms(ref) over the nseq x H outputs of a case.
"""

import math

import pytest
import torch

from vtamiq_amd import _lib
from tests.gpu_util import FORMATS, elt_dtype, num_code, planes_value, stream, to_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG2_SCALE = 0.125 * 1.4426950408889634          # what the engine folds into the query projection of the 3-term formats
FMTS = ["fp16x3", "bf16x3", "fp16", "bf16"]      # {f16, bf16} x {2, 1} planes


def _chunk():
    return _lib.load().vtq_k_cls_fold_chunk_rows()


def _round_up(a, b):
    return (a + b - 1) // b * b


class Case:
    """One set of inputs: x [rows][H] fp32 (nseq sequences of S rows back to back, zero rows behind), LayerNorm and QKV parameters with
    outlier channels, scaled so that the logits reach about +-20."""

    def __init__(self, H, nseq, S, fmt, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.H, self.nseq, self.S, self.fmt, self.nh = H, nseq, S, fmt, H // 64
        self.rows = _round_up(nseq * S, 256) + 256                 # a GEMM row count, with the attention kernel's over-read slack inside
        x = rn(nseq * S, H)
        x[:, [3, H // 2 + 1, H - 5]] *= 30.0                       # outlier channels of the residual stream
        x += 0.5 * rn(1, H)
        self.x = torch.zeros(self.rows, H)
        self.x[: nseq * S] = x
        self.x = self.x.to(DEV)
        self.lw, self.lb = (1.0 + 0.2 * rn(H)).to(DEV), (0.1 * rn(H)).to(DEV)
        a = 2.6 / math.sqrt(H)                                     # |q|, |k| entries ~ 2.6: logits q . k / 8 of std ~ 6.8
        W = torch.cat([a * rn(H, H), a * rn(H, H), rn(H, H) / math.sqrt(H)])
        self.b = torch.cat([0.3 * rn(H), 0.3 * rn(H), 0.3 * rn(H)]).to(DEV)
        self.Wp = to_planes(W.to(DEV), fmt, "w")                   # [wpl][3H][H]
        self.W64 = planes_value(self.Wp)                           # the weights as every kernel reads them
        self.q_log2 = FORMATS[fmt][1] == 3

    def ln64(self):
        x = self.x[: self.nseq * self.S].double().view(self.nseq, self.S, self.H)
        mu = x.mean(-1, keepdim=True)
        var = (x - mu).pow(2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-6) * self.lw.double() + self.lb.double()

    def query(self, token):
        """The fp32 query rows the tail's skinny projection would hand over (log2 units in the 3-term formats)."""
        H = self.H
        q = self.ln64()[:, token] @ self.W64[:H].t() + self.b[:H].double()
        return (q * (LOG2_SCALE if self.q_log2 else 1.0)).float().contiguous()

    def ref(self, q_in=None, token=None):
        """Un-folded fp64: from the kernel's own fp32 query (q_in) or, for the full layer, from the fp64 query of row `token`."""
        H, nh, nseq, S = self.H, self.nh, self.nseq, self.S
        ln = self.ln64()
        k = (ln @ self.W64[H:2 * H].t() + self.b[H:2 * H].double()).view(nseq, S, nh, 64)
        v = (ln @ self.W64[2 * H:].t() + self.b[2 * H:].double()).view(nseq, S, nh, 64)
        if q_in is None:
            q = (ln[:, token] @ self.W64[:H].t() + self.b[:H].double()).view(nseq, nh, 64)
            s = torch.einsum("nhd,nshd->nhs", q, k) * 0.125
            p = torch.softmax(s, -1)
        else:
            s = torch.einsum("nhd,nshd->nhs", q_in.double().view(nseq, nh, 64), k)
            if not self.q_log2:
                s = s * 0.125
            d = s - s.amax(-1, keepdim=True)
            p = torch.exp2(d) if self.q_log2 else torch.exp(d)
            p = p / p.sum(-1, keepdim=True)
        return torch.einsum("nhs,nshd->nhd", p, v).reshape(nseq, H), s

    def fold(self, q_in, x=None, nseq=None):
        lib = _lib.load()
        H, nh, S = self.H, self.nh, self.S
        nseq = nseq or self.nseq
        x = self.x if x is None else x
        apl = 2 if FORMATS[self.fmt][1] > 1 else 1
        chunks = (S + _chunk() - 1) // _chunk()
        u = torch.empty(nseq * nh * H, device=DEV)
        part = torch.empty(nseq * chunks * nh * (H + 2), device=DEV)
        Rz = _round_up(nseq, 64)
        z = torch.zeros((apl, Rz, nh * H), dtype=elt_dtype(self.fmt), device=DEV)
        ctx = torch.zeros(nseq, H, device=DEV)
        _lib.check(lib.vtq_k_cls_fold(q_in.data_ptr(), self.Wp.data_ptr(), 3 * H * H, self.b.data_ptr(), x.data_ptr(), S * H, self.lw.data_ptr(),
                                      self.lb.data_ptr(), nseq, S, H, num_code(self.fmt), 1 if self.q_log2 else 0, u.data_ptr(), part.data_ptr(),
                                      z.data_ptr(), Rz * nh * H, ctx.data_ptr(), stream()))
        torch.cuda.synchronize()
        return ctx

    def full_layer(self, token):
        """The kernels of the full last layer on the same inputs; the attention output row of `token` of every sequence."""
        lib = _lib.load()
        H, S, nseq, rows, fmt = self.H, self.S, self.nseq, self.rows, self.fmt
        f16, terms = FORMATS[fmt]
        apl = 2 if terms > 1 else 1
        dt = elt_dtype(fmt)
        ln = torch.zeros((apl, rows, H), dtype=dt, device=DEV)
        _lib.check(lib.vtq_k_layernorm(self.x.data_ptr(), self.lw.data_ptr(), self.lb.data_ptr(), ln.data_ptr(), rows * H, rows, H, f16, apl, stream()))
        qkv = torch.zeros((apl, rows, 3 * H), dtype=dt, device=DEV)
        _lib.check(lib.vtq_k_gemm(ln.data_ptr(), rows * H, H, self.Wp.data_ptr(), 3 * H * H, rows, 3 * H, H, num_code(fmt), 0, self.b.data_ptr(),
                                  None, None, qkv.data_ptr(), rows * 3 * H, 3 * H, stream()))
        out = torch.zeros((apl, rows, H), dtype=dt, device=DEV)
        _lib.check(lib.vtq_k_attention(qkv.data_ptr(), rows * 3 * H, out.data_ptr(), rows * H, nseq, S, S, H, num_code(fmt), stream()))
        torch.cuda.synchronize()
        return planes_value(out)[: nseq * S].view(nseq, S, H)[:, token]


def _err(got, ref):
    return ((got.double() - ref).abs().max() / ref.pow(2).mean().sqrt()).item()


def _sizes():
    c = _chunk()
    return [2, c - 1, c, c + 1, 2 * c + 3, 501]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H", [768, 1024])
def test_fold_accuracy_against_the_full_layer_kernels(H, fmt):
    """fold error <= 2 x the full-layer kernels' error, case by case: nseq in {2, 3} x S in {2, chunk - 1, chunk, chunk + 1, 2 chunk + 3, 501}
    x consumed token in {0, S - 1}, per (H, format).  Measured on MI355X (chunk = 64; profiles/r08_cls_fold.txt lists all 192 cases),
    error = max |got - fp64| / rms(fp64), range over the 24 cases of each (H, format):
        H     format   fold                    full-layer kernels      worst fold / full-layer of one case
        768   fp16x3   1.08e-06 .. 5.65e-06    3.78e-06 .. 1.16e-05    1.06
        768   bf16x3   1.41e-05 .. 3.44e-05    4.99e-05 .. 2.05e-04    0.45
        768   fp16     6.75e-04 .. 1.28e-03    1.86e-03 .. 1.53e-02    0.44
        768   bf16     6.18e-03 .. 1.39e-02    1.52e-02 .. 6.89e-02    0.58
        1024  fp16x3   1.31e-06 .. 8.65e-06    4.42e-06 .. 1.79e-05    1.11
        1024  bf16x3   1.66e-05 .. 3.17e-05    6.09e-05 .. 2.01e-04    0.47
        1024  fp16     6.81e-04 .. 1.31e-03    1.89e-03 .. 1.06e-02    0.42
        1024  bf16     5.81e-03 .. 1.10e-02    2.52e-02 .. 7.06e-02    0.29
    (the single-plane formats round the query-side K / V and P to 8 / 11 bits in the full layer; the fold keeps them in fp32).
    """
    bad = []
    for nseq in (2, 3):
        for S in _sizes():
            c = Case(H, nseq, S, fmt, seed=1000 + 7 * S + nseq)
            for token in (0, S - 1):
                q_in = c.query(token)
                ref_fold, s = c.ref(q_in=q_in)
                e_fold = _err(c.fold(q_in), ref_fold)
                ref_full, _ = c.ref(token=token)
                e_full = _err(c.full_layer(token), ref_full)
                print(f"cls_fold accuracy H={H} {fmt} nseq={nseq} S={S} token={token}: logits {s.min().item():+.1f}..{s.max().item():+.1f}{' (log2)' if c.q_log2 else ''} "
                      f"fold {e_fold:.2e}  full-layer kernels {e_full:.2e}  ratio {e_fold / e_full:.2f}")
                if not e_fold <= 2.0 * e_full:
                    bad.append((nseq, S, token, e_fold, e_full))
    assert not bad, bad


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16"])
@pytest.mark.parametrize("H,S", [(768, 131), (1024, 65), (768, 501)])
def test_fold_does_not_depend_on_the_batch_and_repeats_bitwise(H, S, fmt):
    """Sequences 0-1 of an nseq = 6 call are the bits of an nseq = 2 call on them; two runs of the same call give identical bits."""
    c = Case(H, 6, S, fmt, seed=5)
    q = c.query(0)
    six, again = c.fold(q), c.fold(q)
    two = c.fold(q[:2].contiguous(), nseq=2)
    assert bool(torch.isfinite(six).all())
    assert torch.equal(six.view(torch.int32), again.view(torch.int32))
    assert torch.equal(six[:2].view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16"])
@pytest.mark.parametrize("H,S", [(768, 131), (1024, 64)])
def test_fold_nan_sequence_stays_alone(H, S, fmt):
    """A sequence of NaN rows (and its NaN query) yields NaN for itself and leaves every other sequence's bits alone."""
    c = Case(H, 5, S, fmt, seed=6)
    q = c.query(S - 1)
    clean = c.fold(q)
    k = 2
    xb, qb = c.x.clone(), q.clone()
    xb[k * S:(k + 1) * S] = float("nan")
    qb[k] = float("nan")
    dirty = c.fold(qb, x=xb)
    for s_ in range(5):
        if s_ == k:
            assert bool(torch.isnan(dirty[s_]).all())
        else:
            assert torch.equal(clean[s_].view(torch.int32), dirty[s_].view(torch.int32)), s_
            assert bool(torch.isfinite(dirty[s_]).all())
    # one NaN row in the middle of a sequence reaches that sequence only, too
    xb = c.x.clone()
    xb[k * S + S // 2, 17] = float("nan")
    dirty = c.fold(q, x=xb)
    assert bool(torch.isnan(dirty[k]).all())
    keep = [s_ for s_ in range(5) if s_ != k]
    assert torch.equal(clean[keep].view(torch.int32), dirty[keep].view(torch.int32))


@pytest.mark.parametrize("fmt", ["fp16x3", "bf16x3"])
def test_fold_huge_logits_give_the_one_hot_limit(fmt):
    """Scores of about 1e4 in log2 units: exp2(s - m) is exact at the maximum and 0 elsewhere, so ctx_h = W_v,h ln_s* + b_v,h for the best
    row s* of each head.  Checked on the (sequence, head) pairs whose best score leads the runner-up by more than 64 (2^-64 is below
    anything fp32 resolves; at these magnitudes a pair of near-tied rows is decided by the rounding of the scores, in any arithmetic) --
    nearly all of them -- and every output is finite.  The only rounding left there is the value projection's: zbar = ln_s* as hi + lo
    planes (2^-22 / 2^-16 relative) against 3-term weights, summed in fp32 -- the bounds of the two-plane formats elsewhere in this suite
    (1e-5 / 2e-4), here relative to the rms."""
    H, S, nseq = 768, 2 * _chunk() + 3, 3
    c = Case(H, nseq, S, fmt, seed=7)
    q = c.query(0)
    _, s = c.ref(q_in=q)
    q = (q * (1.0e4 / s.abs().max().item())).contiguous()
    ref, s = c.ref(q_in=q)
    assert s.abs().max().item() > 9.0e3
    top = s.topk(2, -1).values
    clear = (top[..., 0] - top[..., 1]) > 64.0                             # [nseq][nh]
    assert clear.float().mean().item() > 0.8, clear
    ln = c.ln64()
    best = s.argmax(-1)                                                    # [nseq][nh]
    pick = ln[torch.arange(nseq, device=DEV)[:, None], best]               # [nseq][nh][H]
    onehot = torch.einsum("nhk,hdk->nhd", pick, c.W64[2 * H:].view(c.nh, 64, H)) + c.b[2 * H:].double().view(c.nh, 64)
    assert _err(ref.view(nseq, c.nh, 64)[clear], onehot[clear]) < 1e-12    # the fp64 softmax is one-hot there as well
    got = c.fold(q)
    assert bool(torch.isfinite(got).all())
    e = _err(got.view(nseq, c.nh, 64)[clear], onehot[clear])
    print(f"cls_fold huge logits {fmt}: |score| up to {s.abs().max().item():.3g}, {int(clear.sum())} of {clear.numel()} heads clear, error {e:.2e}")
    assert e < {"fp16x3": 1e-5, "bf16x3": 2e-4}[fmt], e
