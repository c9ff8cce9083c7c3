"""The embedding front end's edge cases and its row-level check (tests/test_gpu_embed.py), shared the way tests/stage_probe.py is -- not a
conftest.  Importing this module needs no GPU: tests/test_embed_cases.py proves on the host what the GPU tests rely on.

Three parts:
  * the CASE BUILDER: positions on and next to every cell border of the G x G positional table (`edge_values`, `edge_rows`, `full_rows`,
    `positions`), the out-of-range positions (`OUT_OF_RANGE`, `clamped_cell`) and the scale ids (`scale_values`), all fp32, deterministic.
    floor(pos * G) is evaluated in the input's dtype by the reference (oracle.pos_index); for some fp32 values just below k / G the fp32
    product rounds up to k while the exact product stays below it (`differing`): a kernel that contracts, reorders or widens that product
    picks another table row there, and a uniform random draw never lands on such a value.
  * the CALLS: every entry that reaches the front end (`Call`), its inputs in the engine's packed patch-row order (`make_inputs`) and
    the expected residual stream, `oracle.embeddings` of each sequence alone placed at its packed row (`expected`).
  * the COMPARISON: `bad_rows` names every row that differs.

Packed order (engine.hip geometry_seq / vtq_forward_varlen): the sequences of image 0 first (references), then image 1, image 2; every
sequence T token rows then its own patches; the packed PATCH rows (what embed_index_kernel indexes) in the same image-major order.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from oracle import vtamiq_oracle as O
from vtamiq_amd import synth
from vtamiq_amd.spec import make_spec

F32 = np.float32

# ---- models: two layers (the stop after stage 0 needs a layer behind it), a one-block head ---------------------------------------------
_HEAD = dict(num_rgs=1, num_rcabs=1, ca_reduction=16)


def _kw(variant, extra, scales):
    return dict(vit_config=dict(variant=variant, num_keep_layers=2, num_extra_tokens=extra, num_scales=scales, pretrained=False), **_HEAD)


MODELS = {
    "b16_t1": _kw("ViT-B16", 0, 0),                 # T = 1, no scale table: the positional row is the only addend
    "b16_t3_s2": _kw("ViT-B16", 2, 2),              # T = 3, 2 scales
    "b16_t9_s3": _kw("ViT-B16", 8, 3),              # T = 9, 3 scales
    "b8_t2_s2": _kw("ViT-B8", 1, 2),                # G = 48, patch K = 192 padded to the GEMM's k-step
    "l16_t1_s3": _kw("ViT-L16", 0, 3),              # H = 1024
}
WSEED = 907


def spec_of(mkey):
    return make_spec(**json.loads(json.dumps(MODELS[mkey])))


_sd = {}


def state_dict(mkey, zero_patch=False):
    """numpy weights of synth.make_state_dict; zero_patch: the patch convolution's weight and bias are zero, so a patch row of the
    embedding output is pos_table[idx] (+ scale_table[sidx]) and nothing else."""
    if (mkey, zero_patch) not in _sd:
        sd = synth.make_state_dict(spec_of(mkey), WSEED)
        if zero_patch:
            for k in ("weight", "bias"):
                sd["transformer.embeddings.patch_embeddings." + k] = np.zeros_like(sd["transformer.embeddings.patch_embeddings." + k])
        _sd[(mkey, zero_patch)] = sd
    return _sd[(mkey, zero_patch)]


# ---- positions ---------------------------------------------------------------------------------------------------------------------------
def edge_values(G: int) -> np.ndarray:
    """The in-range edge positions of a G-cell axis, fp32: just below every border k / G (k >= 1), every border, just above every border,
    every cell centre, and 0, -0, the smallest subnormal, float32(1 - 1e-6) (the loader's clamp) and the largest value below 1."""
    g, k = F32(G), np.arange(G, dtype=F32)
    border = k / g
    below = np.nextafter(border[1:], F32(-1))
    above = np.nextafter(border, F32(2))
    centre = (k + F32(0.5)) / g
    special = np.array([0.0, -0.0, np.nextafter(F32(0), F32(1)), F32(1 - 1e-6), np.nextafter(F32(1), F32(0))], dtype=F32)
    return np.concatenate([below, border, above, centre, special]).astype(F32)


def cell(values, G: int, dtype=torch.float32) -> np.ndarray:
    """floor(v * G) as oracle.pos_index evaluates it in `dtype`, read off the index of the position (v, 0)."""
    v = torch.as_tensor(np.asarray(values, dtype=F32)).to(dtype)
    return ((O.pos_index(torch.stack([v, torch.zeros_like(v)], -1), G) - 1) // G).numpy()


def differing(values, G: int) -> np.ndarray:
    """Mask of the values whose fp32 floor(v * G) is not their fp64 floor."""
    return cell(values, G, torch.float32) != cell(values, G, torch.float64)


def edge_rows(G: int) -> np.ndarray:
    """(2 n + 4, 2) positions: every edge value once in coordinate 0 and once in coordinate 1 (the other coordinate walks through the
    edge values too), then the four corner cells."""
    v = edge_values(G)
    n = len(v)
    other = v[(np.arange(n) * 7 + 3) % n]
    lo, hi = F32(0), np.nextafter(F32(1), F32(0))
    corners = np.array([[lo, lo], [lo, hi], [hi, lo], [hi, hi]], dtype=F32)
    return np.concatenate([np.stack([v, other], 1), np.stack([other, v], 1), corners]).astype(F32)


def full_rows(G: int) -> np.ndarray:
    """(G * G, 2): the centre of every cell, so that every table row 1 .. G * G is addressed."""
    c = (np.arange(G, dtype=F32) + F32(0.5)) / F32(G)
    return np.stack([np.repeat(c, G), np.tile(c, G)], 1).astype(F32)


def positions(G: int, rows: int, full: bool, seed: int) -> np.ndarray:
    """(rows, 2) fp32 in [0, 1): the edge rows (then, `full`, the cell centres) from row 0 on, the rest uniform random as the loader's.
    Fewer rows than edge rows: their first `rows` (just-below-border values first)."""
    e = np.concatenate([edge_rows(G), full_rows(G)]) if full else edge_rows(G)
    if full and rows < len(e):
        raise ValueError(f"{rows} patch rows do not hold the {len(e)} rows of the full edge set")
    fill = np.minimum(np.random.RandomState(seed).uniform(0.0, 1.0, size=(max(rows - len(e), 0), 2)).astype(F32), F32(1.0 - 1e-6))
    return np.concatenate([e, fill])[:rows].astype(F32)


# positions the reference's table lookup does not survive: floor(pos * G) outside [0, G) or NaN.  The smallest negative subnormal times G is
# still a negative subnormal: floor -1.
OUT_OF_RANGE = [("one", 1.0), ("above_one", float(np.nextafter(F32(1), F32(2)))), ("two", 2.0), ("1e30", 1e30), ("minus_1e-9", -1e-9),
                ("minus_subnormal", float(np.nextafter(F32(0), F32(-1)))), ("plus_inf", float("inf")), ("minus_inf", float("-inf")),
                ("nan", float("nan"))]


def clamped_cell(value: float, G: int) -> int:
    """The cell embed_index_kernel gives an out-of-range coordinate (elementwise.hip): floor(v * G) < 0 or NaN -> 0, >= G -> G - 1."""
    f = np.floor(F32(value) * F32(G))
    return 0 if (np.isnan(f) or f < 0) else int(min(f, G - 1))


# ---- scale ids ---------------------------------------------------------------------------------------------------------------------------
def scale_values(ns: int) -> np.ndarray:
    """Every scale id the reference's clamp(scale, 0, ns - 1) + 1 -> long survives (oracle.scale_index); NaN is not one of them."""
    return np.array([*range(ns), 0.5, 0.999999, 1.5, ns - 0.5, -0.0, -0.5, -1, ns, 1e9, np.inf, -np.inf], dtype=F32)


def scales(ns: int, rows: int) -> np.ndarray:
    v = scale_values(ns)
    return v[(np.arange(rows) * 5 + 2) % len(v)]          # 5 and len(v) are coprime for ns = 2, 3: every value within any len(v) rows


# ---- calls -------------------------------------------------------------------------------------------------------------------------------
class Call:
    """One entry call.  kind: forward | pairwise | vit | group | encode | cached | varlen; images: sequences per image (forward (B, B),
    pairwise (B, B, B), vit / encode / cached (B,), group (G, M)); N patches per sequence -- or `lengths` (varlen): the pairs' patch counts."""

    def __init__(self, kind, images=None, N=None, lengths=None, index=None, full=False):
        self.kind, self.images, self.N, self.lengths, self.index, self.full = kind, images, N, lengths, index, full
        if kind == "varlen":
            self.images = (len(lengths), len(lengths))

    def seq_lengths(self):
        """Patch count of every sequence in packed order."""
        if self.kind == "varlen":
            return list(self.lengths) * 2
        return [self.N] * sum(self.images)

    def image_rows(self):
        if self.kind == "varlen":
            return [sum(self.lengths)] * 2
        return [b * self.N for b in self.images]

    def patch_rows(self):
        return sum(self.image_rows())

    def token_rows(self, T):
        return sum(n + T for n in self.seq_lengths())

    def __repr__(self):
        return f"{self.kind}{tuple(self.images)}x{self.lengths if self.kind == 'varlen' else self.N}{' full' if self.full else ''}"


def make_inputs(spec, call: Call, seed: int, tokens_in: bool):
    """-> dict of FLAT numpy arrays over the packed patch rows: p (R, 3, P, P) or (R, H), pos (R, 2), sc (R,) or None."""
    R, P = call.patch_rows(), spec.patch_size
    r = np.random.RandomState(seed)
    p = (0.3 * r.normal(size=(R, spec.hidden_size))).astype(F32) if tokens_in else r.uniform(-1.0, 1.0, size=(R, 3, P, P)).astype(F32)
    return dict(p=p, pos=positions(spec.pos_grid, R, call.full, seed + 1), sc=scales(spec.num_scales, R) if spec.use_scale_embedding else None)


def per_image(call: Call, flat, tail=()):
    """A flat (R, ...) array -> one array per image: (B_k, N, ...), or (sum(lengths), ...) for varlen."""
    if flat is None:
        return [None] * len(call.images)
    out, r0 = [], 0
    for b, rows in zip(call.images, call.image_rows()):
        a = flat[r0:r0 + rows]
        out.append(a if call.kind == "varlen" else a.reshape(b, call.N, *a.shape[1:]))
        r0 += rows
    return out


def expected(sd_t, spec, call: Call, inp, dtype=torch.float32, pos_dtype=torch.float32) -> torch.Tensor:
    """(token rows, H): oracle.embeddings of every sequence alone, at its packed row.  sd_t: torch weights of `dtype`; the patches go in
    as `dtype`, positions as pos_dtype (the reference floors in the input's dtype), scale ids stay fp32."""
    p, pos = torch.as_tensor(inp["p"]).to(dtype), torch.as_tensor(inp["pos"]).to(pos_dtype)
    sc = None if inp["sc"] is None else torch.as_tensor(inp["sc"])
    out, r0 = [], 0
    for n in call.seq_lengths():
        out.append(O.embeddings(sd_t, spec, p[None, r0:r0 + n], pos[None, r0:r0 + n], None if sc is None else sc[None, r0:r0 + n])[0])
        r0 += n
    return torch.cat(out)


def token_row_of_patch(call: Call, T: int, r: int) -> int:
    """The row of the residual stream that packed patch row r is embedded into."""
    row = 0
    for n in call.seq_lengths():
        if r < n:
            return row + T + r
        r -= n
        row += n + T
    raise IndexError(r)


def to_device(call: Call, inp, device="cuda", pos_dtype=None, sc_dtype=None):
    """The per-image device tensors of a call: dict(p, pos, sc) of tuples (sc: tuple of None without a scale table)."""
    def dev(arrs, dt=None):
        return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt) for a in arrs)
    return dict(p=dev(per_image(call, inp["p"])), pos=dev(per_image(call, inp["pos"]), pos_dtype), sc=dev(per_image(call, inp["sc"]), sc_dtype))


def run(model, call: Call, d):
    """Make the entry call on device inputs `d` (to_device).  cached: `d["ref"]` holds the ReferenceFeatures (made on first use)."""
    p, pos, sc = d["p"], d["pos"], d["sc"]
    none = sc[0] is None
    with torch.no_grad():
        if call.kind == "forward":
            return model(p, pos, sc)
        if call.kind == "pairwise":
            return model.forward_pairwise(p, pos, None if none else sc)
        if call.kind == "vit":
            return model.forward_vit(p[0], pos[0], sc[0])
        if call.kind == "group":
            return model.forward_group(p, pos, sc, call.index)
        if call.kind == "encode":
            return model.encode_reference(p[0], pos[0], sc[0])
        if call.kind == "cached":
            if "ref" not in d:                                  # two references of 8 patches at cell centres: in range, no flag
                n, G = 8, model.spec.pos_grid
                dev, g = p[0].device, torch.Generator().manual_seed(5)
                rp = torch.rand(2, n, *p[0].shape[2:], generator=g).to(dev)
                rpos = torch.from_numpy(full_rows(G)[:2 * n].reshape(2, n, 2)).to(dev)
                d["ref"] = model.encode_reference(rp, rpos, None if none else torch.zeros(2, n, device=dev))
            return model.forward_cached(d["ref"], p[0], pos[0], sc[0], call.index)
        if call.kind == "varlen":
            return model.forward_varlen(p, pos, None if none else sc, call.lengths)
    raise ValueError(call.kind)


# every entry that reaches the front end, at shapes whose packed patch rows hold the whole edge set of G = 24 (204 rows).  group: G != M both
# ways (R0 != BN in img_of_row).  varlen: a pair of one patch, the longest pair in the middle, and its patch rows 201 .. 500 cross row 256;
# 1196 patch rows: the full edge set fits
VARLEN_LENGTHS = [1, 200, 300, 90, 7]
ENTRY_CALLS = {
    "forward": Call("forward", (2, 2), 55),
    "pairwise": Call("pairwise", (2, 2, 2), 40),
    "vit": Call("vit", (1,), 210),
    "group_1x5": Call("group", (1, 5), 40, index=[0, 0, 0, 0, 0]),
    "group_3x2": Call("group", (3, 2), 44, index=[2, 0]),
    "encode": Call("encode", (2,), 110),
    "cached": Call("cached", (3,), 77, index=[1, 0, 1]),
    "varlen": Call("varlen", lengths=VARLEN_LENGTHS, full=True),
}
# the smallest shapes of each addressing path: nseq * N = 2 (one GEMM tile of 254 pad rows with row_map = -1), 255 / 256 / 257 (the P_pad seam),
# and one call per grid whose N holds the full edge set (N >= G * G)
SHAPE_CALLS = {
    "rows2": Call("forward", (1, 1), 1),
    "rows255": Call("vit", (3,), 85),
    "rows256": Call("forward", (1, 1), 128),
    "rows257": Call("vit", (1,), 257),
    "full24": Call("forward", (1, 1), 600, full=True),
    "full48": Call("forward", (1, 1), 2400, full=True),
}
# (model, shape call): T = 1, 3, 9; ViT-B/8 (G = 48, K = 192); ViT-L/16 (H = 1024); no / 2 / 3 scales
SHAPE_CASES = [("b16_t1", "rows2"), ("b16_t1", "rows255"), ("b16_t3_s2", "rows256"), ("b16_t9_s3", "rows257"), ("b16_t1", "full24"),
               ("b16_t9_s3", "full24"), ("b8_t2_s2", "rows257"), ("b8_t2_s2", "full48"), ("l16_t1_s3", "rows255"), ("l16_t1_s3", "full24")]


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def bad_rows(got: torch.Tensor, want: torch.Tensor) -> list:
    """Rows of got (R, H) that are not element for element the values of want (a NaN never compares equal)."""
    assert got.shape == want.shape, (got.shape, want.shape)
    return torch.nonzero((got != want).any(-1)).flatten().tolist()
