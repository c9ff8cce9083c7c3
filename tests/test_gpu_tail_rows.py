"""The CLS tail's rows against fp64, per channel, at every row count -- and the difference and the head from caller-held rows.

tests/test_gpu_stages.py measures every encoder stage up to the last layer row by row; behind it the default (pruned) engine runs
rows_ln -> query projection -> cls_fold -> value projection -> out-proj -> rows_ln -> fc1 -> fc2 (cls_tail.hip, skinny.hip) with no stop
point, then the difference kernel and the head.  Their row count is the call's SEQUENCE count, and launch_skinny changes kernel form
(16 / 32 / 64 rows per workgroup, one or several row workgroups) with it: tests/tail_rows.py lists the counts on either side of every
switch.  No debug entry is needed to see the tail's output: encode_reference() returns, per image, the consumed token's residual row behind
the last layer (before encoder_norm), and forward_cached() takes such rows back and runs group_diff and the head on them.

  * test_tail_rows / test_tail_rows_ragged: ONE two-layer model per (case, mode, last-layer path); the catalogue's sequence counts in
    listed order, then reversed (workspace growth; stale rows behind a smaller call), 8 patches per image.  The stream entering the last
    layer is taken with vtq_debug_stop_after (StageProbe), the exported rows are compared with test_gpu_stages.tail_rows_ref of that
    stream -- the model's own fp32 weights in fp64 -- by stage_probe.row_error: max over channels of |got - ref| / rms(ref row).
    The full last layer (OPT_FULL_LAST_LAYER), whose stages STAGE_BOUND already checks, is the independent yardstick for the same rows.
  * test_cached_rows_to_scores: forward_cached on rows the TEST holds (other images' rows, a row with one outlier channel, a constant
    row) against the fp64 head on gamma * (LN(ref row) - LN(dist row)), at the head's row counts, under test_gpu_kernels.HEAD_TOL.
  * test_row_check_sees_what_the_score_cannot: one fc2 weight moved in the reference's copy.

TAIL_ROW_BOUND: per mode about 3x the worst row observed on the MI355X against that fp64 reference over every case, path, G, sequence and
both call forms, never above the ceilings of test_gpu_stages.py (fp16x3 5e-5, bf16x3 5e-4, fp16x2 5e-3, fp16 2e-2, bf16 1e-1).  Observed
(profiles/r21_tail_rows.txt has every (case, G); VTQ_TAIL_ROWS_TABLE=<path> writes it), worst row, CLS-only tail | full last layer:
            vitb                 vitb_stress          refdefault           vitl                 bound
  fp16x3    4.8e-6 | 5.8e-6      5.6e-6 | 6.9e-6      5.0e-6 | 6.1e-6      4.9e-6 | 6.2e-6      2e-5
  bf16x3    2.7e-5 | 2.5e-5      3.6e-5 | 4.3e-5      2.4e-5 | 2.7e-5                           1.3e-4
  fp16x2    1.0e-3 | 1.0e-3      1.8e-3 | 1.8e-3      1.1e-3 | 1.1e-3                           5e-3 (3x is 5.4e-3: the ceiling)
  fp16      1.6e-3 | 1.6e-3      2.5e-3 | 2.8e-3      1.8e-3 | 1.7e-3                           8e-3
  bf16      1.2e-2 | 1.2e-2      2.3e-2 | 2.5e-2      1.4e-2 | 1.4e-2      1.3e-2 | 1.3e-2      7.5e-2
The CLS-only tail never exceeds the full last layer by more than 1.1x (it rounds neither K, V nor the LayerNorm rows to planes).  The worst
row of a call is one and the same (sequence, channel) from the count at which that sequence enters the call onwards -- across 16 | 17,
80 | 81, 160 | 161 -- so the error does not step at a switch of the rows-per-workgroup rule and does not gather in the last rows of a row
block; a call behind a larger one returns the bits of the same call on the way up (asserted).  fp16x2's rows are the fp32 residual plus
a two-term product: its error is the dropped weight plane's, the same on both paths.

The head from caller-held rows (HEAD_TOL = 2e-5 * max(1, |ref|), unchanged): worst |q - ref| 1.0e-5 (ViT-B, at constant reference rows,
M = 672 / 673), 1.9e-6 (ViT-L); the same figures on both last-layer paths and in fp16x3 and bf16 -- the head runs fp16 hi / lo planes
whatever the encoder's mode.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests import tail_rows as R
from tests.helpers import gate_error, stress_state
from tests.stage_probe import RefWeights, StageProbe, row_error
from tests.test_gpu_kernels import HEAD_TOL
from tests.test_gpu_stages import TAIL_BOUND, build, tail_ref, tail_rows_ref, tail_scores
from vtamiq_amd import _lib, synth
from vtamiq_amd.model import ReferenceFeatures
from vtamiq_amd.spec import make_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = 8                                                    # patches per image
ALL_MODES = ["fp16x3", "bf16x3", "fp16x2", "fp16", "bf16"]
PATHS = {"pruned": 0, "full": _lib.OPT_FULL_LAST_LAYER}

# max_c |got - ref| / rms(ref row) of an exported row; the module docstring has what it was measured against and the observed table
TAIL_ROW_BOUND = {"fp16x3": 2e-5, "bf16x3": 1.3e-4, "fp16x2": 5e-3, "fp16": 8e-3, "bf16": 7.5e-2}

_REFDEFAULT = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_extra_tokens=8, use_layer_scale=True, num_scales=0), ca_reduction=16)
CASES = {
    # name: (kwargs, weight seed, stress_state arguments or None, token_num, catalogue configuration, modes)
    "vitb": (dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2)), 71, None, 0, R.VIT_B, ALL_MODES),
    "vitb_stress": (dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2)), 72, dict(qk=5.0, head=True), 0, R.VIT_B, ALL_MODES),
    "refdefault": (_REFDEFAULT, 73, None, 8, R.VIT_B, ALL_MODES),          # token_num = the last of the 8 register tokens
    "vitl": (dict(vit_config=dict(variant="ViT-L16", num_keep_layers=2, num_scales=3)), 74, None, 0, R.VIT_L, ["fp16x3", "bf16"]),
}
_cache = {}
_table = {}                                               # (case, mode, path, what, G) -> (worst row error, sequence, channel)


def get_case(name, images):
    """Host weights, fp64 GPU weights and `images` single images (device tensors) of a case; one case at a time."""
    key = (name, images)
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        kw, wseed, stress, token, cfg, _ = CASES[name]
        kw = json.loads(json.dumps(kw))
        kw["vit_config"]["pretrained"] = False
        spec = make_spec(**json.loads(json.dumps(kw)))
        sd = stress_state(spec, wseed, **stress) if stress else synth.make_state_dict(spec, wseed)
        patches, pos, scales = synth.make_inputs(spec, (images + 1) // 2, NP, 900 + wseed, aligned=False)
        dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV, torch.float32).flatten(0, 1)[:images].contiguous()
        _cache[key] = dict(kw=kw, spec=spec, sd=sd, sdr=RefWeights(sd), token=token, cfg=cfg, patches=dev(patches), pos=dev(pos), scales=dev(scales))
    return _cache[key]


def image_args(c, G):
    return c["patches"][:G], c["pos"][:G], (c["scales"][:G] if c["scales"] is not None else None)


def ragged_args(c, lens):
    """The first lens[j] patches of image j, concatenated: the (sum(lengths), ...) form of a `lengths=` call."""
    cat = lambda t: None if t is None else torch.cat([t[j, :n] for j, n in enumerate(lens)]).contiguous()
    return cat(c["patches"]), cat(c["pos"]), cat(c["scales"])


@pytest.fixture(scope="module", autouse=True)
def rows_table():
    """With VTQ_TAIL_ROWS_TABLE=<path> in the environment the per-(case, G) table of this run is written there (profiles/r21_tail_rows.txt
    is one), behind the '#' lines an existing file begins with."""
    yield
    path = os.environ.get("VTQ_TAIL_ROWS_TABLE")
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
            f.write("case          mode    path    call      G     worst row    sequence  channel\n")
            for (case, mode, path_, what, G), (err, s, ch) in sorted(_table.items(), key=lambda kv: (kv[0][0], ALL_MODES.index(kv[0][1]), kv[0][2], kv[0][3], kv[0][4])):
                f.write(f"{case:<13} {mode:<7} {path_:<7} {what:<9} {G:<5} {err:<12.3e} {s:<9} {ch}\n")


# ---- the measurement ---------------------------------------------------------------------------------------------------

class RowCheck:
    """Exported rows against reference rows, call by call: every row over the bound is kept as (G, sequence, channel, error) and asserted
    at the end, so one run names every bad row count."""

    def __init__(self, case, mode, path, bound, record=True):
        self.key, self.bound, self.misses, self.worst, self.record = (case, mode, path), bound, [], (0.0, None), record

    def check(self, what, G, rows, xr):
        assert rows.shape == xr.shape and rows.dtype == torch.float32, (rows.shape, xr.shape, rows.dtype)
        e, col = row_error(rows, xr)
        for s in torch.nonzero(~(e <= self.bound)).flatten().tolist():
            self.misses.append((what, G, s, int(col[s]), float(e[s])))
        s = int(torch.argmax(e))
        w = (float(e[s]), s, int(col[s]))
        k = self.key + (what, G)
        if self.record and (k not in _table or not w[0] <= _table[k][0]):
            _table[k] = w
        if not w[0] <= self.worst[0]:
            self.worst = (w[0], (what, G, s, w[2]))
        return e

    def measured(self):
        case, mode, path = self.key
        v, where = self.worst
        print(f"measured {case} {mode} {path}: worst row {v:.2e} at (call, G, sequence, channel) = {where}   bound {self.bound:g}")

    def assert_ok(self):
        assert not self.misses, "\n".join(f"{self.key}: {what} G = {G}: sequence {s}, channel {ch}: row error {e:.3e} > {self.bound:g}"
                                          for what, G, s, ch, e in self.misses[:40]) + f"\n({len(self.misses)} rows over the bound)"


def stream_in(model, call, G, N):
    """The residual stream entering the last layer of one encode_reference call of G sequences: rows of x, fp32 on the device."""
    L = model.spec.num_layers
    pr = StageProbe(model, None, G, N, nimg=1, call=call)
    return pr, pr.grab_stop((L - 2) * 7 + 6, want=("x",))["x"]


def uniform_rows(model, c, G):
    """-> (exported rows [G, H], the stream entering the last layer [G, S, H]) of encode_reference on the first G images."""
    call = lambda: model.encode_reference(*image_args(c, G))
    pr, x = stream_in(model, call, G, NP)
    with torch.no_grad():
        rows = call().rows
    return rows, pr.seqs(x)


def _params(names):
    return [pytest.param(n, mode, p, id=f"{n}-{mode}-{p}") for n in names for mode in CASES[n][5] for p in PATHS]


@pytest.mark.parametrize("name,mode,path", _params(CASES))
def test_tail_rows(name, mode, path):
    """Every catalogue count, ascending then descending, on one engine: exported rows against fp64 from the engine's own stream."""
    counts = R.tail_catalogue(**CASES[name][4])
    c = get_case(name, counts[-1])
    spec, t = c["spec"], c["token"]
    model = build(c, mode, PATHS[path], token_num=t)
    chk = RowCheck(name, mode, path, TAIL_ROW_BOUND[mode])
    ref, first = {}, {}
    for G in counts:
        rows, x = uniform_rows(model, c, G)
        ref[G], first[G] = tail_rows_ref(c["sdr"], spec, x.double(), t), rows
        chk.check("uniform", G, rows, ref[G])
    for G in counts[::-1]:                                 # a smaller call behind a larger one: same bits as on the way up
        with torch.no_grad():
            rows = model.encode_reference(*image_args(c, G)).rows
        chk.check("uniform", G, rows, ref[G])
        assert torch.equal(rows, first[G]), f"G = {G}: the rows of a call behind a larger one differ from the same call's on a fresh workspace"
    model.check_inputs()
    chk.measured()
    chk.assert_ok()


@pytest.mark.parametrize("name,mode,path", _params(["vitb", "refdefault"]))
def test_tail_rows_ragged(name, mode, path):
    """encode_reference(lengths=...): 81 and 161 images of 1 .. 8 patches in turn -- rows_ln with the row table, cls_fold with VarSeq."""
    c = get_case(name, R.tail_catalogue(**CASES[name][4])[-1])
    spec, t, T = c["spec"], c["token"], c["spec"].num_tokens
    model = build(c, mode, PATHS[path], token_num=t)
    chk = RowCheck(name, mode, path, TAIL_ROW_BOUND[mode])
    for G in (81, 161, 81):
        lens = R.ragged_lengths(G, NP)
        args = ragged_args(c, lens)
        call = lambda: model.encode_reference(*args, lengths=lens)
        _, x = stream_in(model, call, G, NP)               # (sized for G full sequences: no fewer rows than the call packs)
        with torch.no_grad():
            rows = call().rows
        row0 = R.row_offsets(lens, T)
        xr = torch.empty(G, spec.hidden_size, dtype=torch.float64, device=DEV)
        for n in sorted(set(lens)):                        # the reference per sequence; sequences of one length as one batch
            js = [j for j in range(G) if lens[j] == n]
            xs = torch.stack([x[row0[j]:row0[j] + n + T] for j in js]).double()
            xr[js] = tail_rows_ref(c["sdr"], spec, xs, t)
        chk.check("ragged", G, rows, xr)
    model.check_inputs()
    chk.measured()
    chk.assert_ok()


# ---- difference and head from caller-held rows ---------------------------------------------------------------------------

def chosen_reference_rows(pool, M):
    """M reference rows the test holds, in turn: the exported row of another image; a copy of one with one outlier channel of 30x the
    row's RMS; a constant row (variance 0: its LayerNorm is the bias exactly)."""
    H = pool.shape[1]
    rows = pool[[(m + 7) % pool.shape[0] for m in range(M)]].clone()
    for m in range(1, M, 3):
        rows[m, (37 * m) % H] = 30.0 * float(rows[m].double().pow(2).mean().sqrt()) * (-1.0 if m & 1 else 1.0)
    rows[2::3] = 1.0
    return rows.contiguous()


def head_ref(sd64, spec, ref_rows, dist_rows):
    """fp64: q_predictor(quality_decoder(gamma * (LN(ref) - LN(dist)))) from the two fp32 rows."""
    w, b = sd64["transformer.encoder.encoder_norm.weight"], sd64["transformer.encoder.encoder_norm.bias"]
    d = O._layer_norm(ref_rows.double(), w, b) - O._layer_norm(dist_rows.double(), w, b)
    if spec.diff_scale:
        d = d * sd64["diff_scale.gamma"]
    return O.q_predictor(sd64, O.quality_decoder(sd64, spec, d))


@pytest.mark.parametrize("name,mode", [("vitb", "fp16x3"), ("vitb", "bf16"), ("vitb_stress", "fp16x3"), ("vitl", "fp16x3")])
@pytest.mark.parametrize("path", PATHS)
def test_cached_rows_to_scores(name, mode, path):
    """forward_cached at every head row count: group_diff and the head through the planes_ready path every scoring entry takes."""
    counts = R.head_catalogue(**CASES[name][4])
    c = get_case(name, counts[-1])
    spec = c["spec"]
    model = build(c, mode, PATHS[path], token_num=c["token"])
    sd64 = {k: v.to(DEV) for k, v in O.to_torch(c["sd"], torch.float64).items()}
    with torch.no_grad():
        enc = model.encode_reference(*image_args(c, counts[-1]))
        pool = enc.rows.clone()
        worst, misses = (0.0, None, 0.0, 0.0), []
        for M in counts + counts[::-1]:
            dist_rows = model.encode_reference(*image_args(c, M)).rows          # the distorted images' own rows, as this call size exports them
            ref_rows = chosen_reference_rows(pool, M)
            held = ReferenceFeatures(ref_rows, enc.precision, enc.token, enc.engine_options, enc.signature)
            q = model.forward_cached(held, *image_args(c, M))[0].double()
            ref = head_ref(sd64, spec, ref_rows, dist_rows)
            err = torch.nan_to_num((q - ref).abs(), nan=math.inf)
            tol = HEAD_TOL * max(1.0, float(ref.abs().max()))
            m = int(err.argmax())
            if not float(err[m]) <= worst[0]:
                worst = (float(err[m]), (M, m, ("other image", "outlier channel", "constant row")[m % 3]), float(ref[m]), float(ref.abs().max()))
            misses += [(M, i, float(err[i]), tol) for i in torch.nonzero(~(err < tol)).flatten().tolist()]
    model.check_inputs()
    print(f"measured {name} {mode} {path}: head from caller-held rows, worst |q - ref| {worst[0]:.2e} at (M, image, reference row) = {worst[1]}, ref {worst[2]:.3g} "
          f"(max |ref| {worst[3]:.3g})   bound {HEAD_TOL:g} * max(1, |ref|)")
    assert not misses, "\n".join(f"M = {M}, image {i}: |q - ref| = {e:.3e} >= {tol:.3e}" for M, i, e, tol in misses[:40])


# ---- the check can fail --------------------------------------------------------------------------------------------------

def perturbed_fc2(name, mode, G=64):
    """Figures of the experiment below on the first G images of a case, as G / 2 (reference, distorted) pairs."""
    c = get_case(name, R.tail_catalogue(**CASES[name][4])[-1])
    spec, t, sdr = c["spec"], c["token"], c["sdr"]
    B, bound, H = G // 2, TAIL_ROW_BOUND[mode], c["spec"].hidden_size
    model = build(c, mode, 0, token_num=t)
    rows, x = uniform_rows(model, c, G)
    x = x.double()
    pre = f"transformer.encoder.layers.{spec.num_layers - 1}."
    key = pre + "ffn.fc2.weight"
    # W2[ch, j] += delta moves channel ch of row s by ls2_ch * delta * h[s, j], h = the fc1 + GELU rows fc2 consumes: take the hidden unit
    # with the largest activation and the row it reaches hardest, relative to the row's RMS ...
    xr, h = tail_rows_ref(sdr, spec, x, t, hidden=True)
    j = int(h.abs().amax(0).argmax())
    reach = h[:, j].abs() / xr.pow(2).mean(-1).sqrt()
    s = int(reach.argmax())
    # ... and of 16 channels the one whose move changes the fp64 SCORES least (a choice made in the reference alone)
    q0 = tail_scores(sdr, spec, xr, B)

    def moved_rows(ch):
        ls = float(sdr[pre + "ls2.gamma"][ch]) if spec.use_layer_scale else 1.0
        delta = 8.0 * bound / (float(reach[s]) * abs(ls))
        xr2 = xr.clone()
        xr2[:, ch] += ls * delta * h[:, j]
        return delta, xr2

    ch = min(range(5, H, H // 16), key=lambda k: gate_error(tail_scores(sdr, spec, moved_rows(k)[1], B).cpu().numpy(), q0.cpu().numpy()))
    delta = moved_rows(ch)[0]
    sd2 = dict(c["sd"])
    sd2[key] = c["sd"][key].copy()
    sd2[key][ch, j] += delta
    print(f"\n[{name} {mode}] {key}[{ch}, {j}] += {delta:.3e} (weight rms {float(np.sqrt(np.mean(c['sd'][key] ** 2))):.3e})")
    q2, xr2 = tail_ref(RefWeights(sd2), spec, x, B, t, rows=True)
    ok, bad = RowCheck(name, mode, "unperturbed", bound, record=False), RowCheck(name, mode, "perturbed", bound, record=False)
    ok.check("uniform", G, rows, xr)
    e = bad.check("uniform", G, rows, xr2)
    # the score level: what the fp64 scores of the same images do, and the engine's scores of the G / 2 pairs against the perturbed reference
    args = tuple((a[:B], a[B:G]) if a is not None else (None, None) for a in image_args(c, G))
    with torch.no_grad():
        q = model(*args)[0].cpu().numpy()
    moved, seen = gate_error(q2.cpu().numpy(), q0.cpu().numpy()), gate_error(q, q2.cpu().numpy())
    print(f"   row {s}: error {float(e[s]):.2e} = {float(e[s]) / bound:.1f} x the bound; fp64 scores move by {moved:.2e}; the engine's scores against the "
          f"perturbed reference: gate error {seen:.2e} (against the unperturbed one {gate_error(q, q0.cpu().numpy()):.2e})   bound {TAIL_BOUND[mode]:g}")
    return dict(ok=ok, bad=bad, e=e, s=s, ch=ch, bound=bound, moved=moved, seen=seen)


def test_row_check_sees_what_the_score_cannot():
    """One element of the last layer's fc2 weight moved in the fp64 reference's copy, by an amount that puts the worst affected row at about
    8x its bound: the row check names exactly that channel, while the fp64 scores of the same images move by less than TAIL_BOUND and the
    score-level comparison of test_cls_tail_teacher_forced passes against the perturbed reference."""
    mode = "fp16x3"
    f = perturbed_fc2("vitb_stress", mode)
    ok, bad, e, s, bound = f["ok"], f["bad"], f["e"], f["s"], f["bound"]
    assert not ok.misses, ok.misses
    assert bad.misses and {m[3] for m in bad.misses} == {f["ch"]}, bad.misses             # every row over the bound, at exactly that channel
    assert int(torch.argmax(e)) == s and 6.0 * bound < float(e[s]) < 10.0 * bound, (s, float(e[s]), bound)
    assert f["moved"] < TAIL_BOUND[mode] and f["seen"] <= TAIL_BOUND[mode], (f["moved"], f["seen"])
