"""Teacher-forced stage checks of the encoder (tests/test_gpu_stages.py), shared the way tests/helpers.py is -- not a conftest.

Two halves:
  * `row_error` / `StageLog` (CPU or GPU tensors): the per-TOKEN-ROW error max_c |got - ref| / rms(ref_row).  A row is
    normalised by its own RMS, not by the tensor's max, so one corrupted row, one 256-row tile seam or one sequence that straddles
    a tile stands out even when a score -- the CLS row after 12 layers of attention, an average over ~500 rows -- barely moves.
  * `StageProbe` (GPU): vtq_debug_stop_after / vtq_debug_buffers of the product library.  `grab(layer, stage)` runs one forward
    that leaves the encoder after stage `layer * 7 + stage` and copies the residual stream `x`, the LayerNorm / attention planes
    `lnbuf` and the QKV / MLP planes `big` into torch tensors ON THE DEVICE, decoded with the layouts of DESIGN.md section 3.

Stages of layer i (engine.hip run_encoder): 0 LayerNorm 1 -> lnbuf, 1 QKV -> big (ld 3H), 2 attention -> lnbuf, 3 out-proj
(+ LayerScale, + adapter delta) -> x, 4 LayerNorm 2 -> lnbuf, 5 fc1 + GELU -> big (ld mlp_dim), 6 fc2 (+ LayerScale, + adapter
delta) -> x.  Sequences are packed at pitch S = N + T (engine.hip geometry()), ref images first.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from tests.gpu_util import planes_value
from vtamiq_amd import _lib

STAGES = ["ln1", "qkv", "attn", "x_attn", "ln2", "fc1", "x_mlp"]       # index = stage number k of layer * 7 + k
# modes whose attention takes Q in log2 units: the engine multiplies the query rows of W_qkv and b_q by log2(e) / 8 at ingestion
# (engine.hip kQLog2Scale); the single-plane modes apply 1/8 inside the kernel
THREE_TERM_ATTENTION = ("fp16x3", "bf16x3", "fp16x2")
Q_LOG2_SCALE = 0.125 * math.log2(math.e)
ACT_PLANES = {"fp16x3": 2, "bf16x3": 2, "fp16x2": 2, "fp16": 1, "bf16": 1}


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# ---- the comparator ----------------------------------------------------------------------------------------------------

def row_error(got: torch.Tensor, ref: torch.Tensor):
    """got, ref [..., rows, W] -> (err [..., rows], col [..., rows]): per row max_c |got - ref| / rms(ref_row) and the column of
    that maximum.  A non-finite element makes its row's error +inf (a NaN must never compare as "within bound")."""
    ref = ref.double()
    d = (got.double() - ref).abs()
    m, col = torch.nan_to_num(d, nan=math.inf).max(-1)
    rms = ref.pow(2).mean(-1).sqrt().clamp_min(1e-300)
    return m / rms, col


def global_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The whole-tensor metric max |got - ref| / max |ref| -- what the per-kernel tests use; kept for the comparison only."""
    d = torch.nan_to_num((got.double() - ref.double()).abs(), nan=math.inf)
    return float(d.max() / ref.double().abs().max())


def worst_row(got: torch.Tensor, ref: torch.Tensor):
    """got, ref [nseq, S, W] -> (worst per-row error, (sequence, token, column)) of the whole tensor."""
    e, col = row_error(got, ref)
    flat = int(torch.argmax(e))
    s, t = divmod(flat, e.shape[-1])
    return float(e.reshape(-1)[flat]), (s, t, int(col[s, t]))


class StageLog:
    """Worst rows of a walk over (layer, stage) comparisons: every stage is measured and printed before anything fails, then
    `assert_ok` names each stage over its bound with its worst (layer, stage, sequence, token, column)."""

    def __init__(self, tag: str):
        self.tag, self.rec = tag, []                                 # (layer, stage, worst, (sequence, token, column), bound)

    def check(self, layer: int, stage: str, got: torch.Tensor, ref: torch.Tensor, bound: float) -> float:
        v, loc = worst_row(got, ref)
        self.rec.append((layer, stage, v, loc, bound))
        print(f"   [{self.tag}] layer {layer:2d} {stage:7s} worst row {v:.2e} at (seq {loc[0]}, token {loc[1]}, column {loc[2]})"
              f"   bound {bound:.2g}{'' if v <= bound else '   <-- OVER'}")
        return v

    def fail(self, layer: int, stage: str, what: str):
        self.rec.append((layer, stage, math.inf, (-1, -1, -1), 0.0))
        print(f"   [{self.tag}] layer {layer:2d} {stage:7s} {what}   <-- FAIL")

    def over(self) -> list:
        return [r for r in self.rec if not r[2] <= r[4]]

    def assert_ok(self):
        assert not self.over(), "\n".join(
            f"{self.tag}: layer {l} {st}: row error {v:.3e} > {b:.2g} at sequence {loc[0]}, token {loc[1]}, column {loc[2]}"
            for l, st, v, loc, b in self.over())


# ---- the probe ---------------------------------------------------------------------------------------------------------

class StageProbe:
    """The product library's workspace after a given encoder stage.  `args` = the model's forward arguments (kept: every grab
    re-runs the same forward -- forwards are bit-deterministic, so the stage outputs of separate grabs belong to one computation).
    `call` (tests/test_gpu_embed.py): a callable that makes another entry call on `model` instead of model(*args); B, N, nimg then only
    say how many rows the call packs (nimg * B sequences of N + T rows)."""

    def __init__(self, model, args, B: int, N: int, nimg: int = 2, call=None):
        if model.precision not in ACT_PLANES:
            raise ValueError(f"StageProbe needs an explicit precision (one of {sorted(ACT_PLANES)}), not {model.precision!r}")
        self.m, self.args, self.spec = model, args, model.spec
        self.call = call if call is not None else (lambda: model(*args))
        self.mode = model.precision
        self.H, self.Md = self.spec.hidden_size, self.spec.mlp_dim
        self.W = max(3 * self.H, self.Md)                            # `big` row width
        self.S, self.nseq = N + self.spec.num_tokens, nimg * B
        self.M_pad = round_up(self.nseq * self.S, 256)               # engine.hip geometry(): the GEMM row count
        self.rows_live = self.M_pad + 128                            # + the attention kernel's over-read slack
        self.planes = ACT_PLANES[self.mode]
        self.dtype = torch.float16 if self.mode.startswith("fp16") else torch.bfloat16
        self.lib, self.hip = _lib.load(), C.CDLL("libamdhip64.so")
        with torch.no_grad():
            self.call()                                              # creates the engine and its workspace
        torch.cuda.synchronize()

    def _copy(self, ptr: int, nbytes: int) -> torch.Tensor:
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        assert self.hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3) == 0   # device to device
        return t

    def grab(self, layer: int, stage: int, want=("x", "ln", "big")) -> dict:
        """Run the forward up to stage `layer * 7 + stage`; copy the live rows of the requested buffers (device tensors)."""
        if layer >= self.spec.num_layers - 1 and self.m.engine_options & _lib.OPT_FULL_LAST_LAYER == 0:
            raise ValueError("the last layer runs the CLS-only tail (cls_tail.hip), which has no stage stops")
        return self.grab_stop(layer * 7 + stage, want)

    def grab_stop(self, stop: int, want=("x", "ln", "big")) -> dict:
        m = self.m
        try:
            _lib.check(self.lib.vtq_debug_stop_after(m._engine, stop))
            with torch.no_grad():
                self.call()                                          # (the head still runs, on stale rows: its scores are ignored)
            torch.cuda.synchronize()
        finally:
            _lib.check(self.lib.vtq_debug_stop_after(m._engine, -1))
        x, ln, big, rows = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(self.lib.vtq_debug_buffers(m._engine, C.byref(x), C.byref(ln), C.byref(big), C.byref(rows)))
        R, H, W, live = rows.value, self.H, self.W, self.rows_live
        assert R >= live, (R, live)
        out = {}
        if "x" in want:
            out["x"] = self._copy(x.value, live * H * 4).view(torch.float32).view(live, H)
        if "ln" in want:                                             # [planes][R][H]: plane stride R * H
            out["ln"] = torch.stack([self._copy(ln.value + p * R * H * 2, live * H * 2).view(self.dtype) for p in range(self.planes)])
        if "big" in want:                                            # [planes][R][W]: plane stride R * W, rows of ld 3H or mlp_dim
            out["big"] = torch.stack([self._copy(big.value + p * R * W * 2, live * W * 2).view(self.dtype) for p in range(self.planes)])
        return out

    # ---- decoders: [nseq, S, width] of the sequences' rows (fp64 for planes: hi + lo) ----
    def seqs(self, t: torch.Tensor) -> torch.Tensor:
        return t[:self.nseq * self.S].reshape(self.nseq, self.S, -1)

    def x(self, st: dict) -> torch.Tensor:
        return self.seqs(st["x"])

    def ln(self, st: dict) -> torch.Tensor:
        return self.seqs(planes_value(st["ln"].view(self.planes, self.rows_live, self.H)))

    def big(self, st: dict, ld: int) -> torch.Tensor:
        n = self.nseq * self.S
        return planes_value(st["big"][:, :n * ld]).view(self.nseq, self.S, ld)

    def pad_rows_finite(self, st: dict) -> list:
        """Names of the buffers whose rows nseq * S ... M_pad + 128 hold a non-finite value.  The attention kernel's last key tile and
        query block read into these rows (engine.hip, above the `big` memset) and rely on them being finite; `big` is checked in both of
        its row layouts (QKV, ld 3H; MLP hidden, ld mlp_dim)."""
        n, live, bad = self.nseq * self.S, self.rows_live, []
        if "x" in st and not bool(torch.isfinite(st["x"][n:live]).all()):
            bad.append("x")
        if "big" in st:
            for ld in (3 * self.H, self.Md):
                if not bool(torch.isfinite(st["big"][:, n * ld:live * ld]).all()):
                    bad.append(f"big (ld {ld})")
        return bad


class RefWeights(dict):
    """{state-dict key: fp64 tensor on the GPU}, converted from the fp32 numpy state dict on first use: the reference reads the
    model's own fp32 weights (not the engine's split planes), so the engine's weight ingestion is checked with every stage."""

    def __init__(self, sd_np, device="cuda"):
        super().__init__()
        self.sd_np, self.device = sd_np, device

    def __missing__(self, k):
        v = torch.as_tensor(self.sd_np[k]).to(device=self.device, dtype=torch.float64)
        self[k] = v
        return v
