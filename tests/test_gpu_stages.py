"""Teacher-forced stage parity of the encoder at production shapes, row by row.

Every stage output the engine writes is compared with an fp64 torch computation ON THE GPU of the same operation, from that stage's
own input as the engine produced it (vtq_debug_stop_after, tests/stage_probe.py), with the model's fp32 weights in fp64 -- not the
engine's split planes, so weight ingestion is checked too.  The error is per TOKEN ROW (max over the row / the row's RMS) over every
row of every sequence: a score is the CLS row after L layers of attention, an average over ~500 rows, so a kernel that corrupts one
row, one 256-row tile seam or the rows behind the last sequence moves it by far less than any score gate resolves.

Each case exists for the kernel path the library's rules pick for it:
  c2_b32_n500          ViT-B/16 L = 12, B = 32, N = 500 (bench.py's shape): persistent 256 x 256 GEMM, pipelined attention, 64 sequences
  stress5h_b32_n500    the same shape on tests.helpers.stress_state weights (peaked softmax, outlier channels ~30x the row RMS)
  c2shape_b2_n500      B = 2: gemm_st 64 / 128 tiles and the 4-wave attention kernel
  refdefault_b16_n512  the reference-default topology (8 registers, LayerScale), S = 521: 256-row query blocks would pad > 15 %, so the
                       3-term modes run the 4-wave kernel at 32 sequences (attention.hip attention_rule)
  vitl_b4_n1024        ViT-L/16 over 3 scales: H = 1024, 16 heads, K = 1024 / 4096
  vitb8_b3_n77         ViT-B/8 (patch K = 192, padded), registers, one adapter pair: nseq * S = 480, not a multiple of 256

  vitb_b81_n8          (the tail check only) 81 pairs of 8 patches: 162 sequences, more rows than any other engine-level case gives the tail

The CLS-only last layer (cls_tail.hip: rows_ln_kernel, cls_fold, the skinny query / value / out-proj / fc1 / fc2), final_diff_kernel and
the skinny head have no stage stops.  Here their SCORES are compared with fp64 from the engine's own stream entering the last layer, at
production size (test_cls_tail_teacher_forced); the tail's ROWS -- what encode_reference() exports -- are measured per sequence and
channel against the same fp64 reference in tests/test_gpu_tail_rows.py, at every row count at which launch_skinny changes kernel form, and
the difference and the head from caller-held rows there too.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import vtamiq_oracle as O
from tests.helpers import gate_error, load_case, split_inputs, stress_state
from tests.stage_probe import Q_LOG2_SCALE, STAGES, THREE_TERM_ATTENTION, RefWeights, StageLog, StageProbe, worst_row
from vtamiq_amd import VTAMIQ, _lib, synth
from vtamiq_amd.spec import make_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_MODES = ["fp16x3", "bf16x3", "fp16x2", "fp16", "bf16"]

# Per-row error bounds, (mode, stage): max_c |got - ref| / rms(ref_row), ref = fp64 of the engine's own stage input, at about 3x the worst
# row observed on the MI355X over every case, layer and row (profiles/r08_stage_parity.txt), never above the ceilings
# fp16x3 5e-5, bf16x3 5e-4, fp16x2 5e-3, fp16 2e-2, bf16 1e-1.  Observed (embed, ln1, qkv, attn, x_attn, ln2, fc1, x_mlp):
#   fp16x3  6.7e-6  6.0e-6  8.0e-6  2.6e-5  5.6e-6  4.6e-6  1.3e-5  8.8e-6
#   bf16x3  2.7e-5  1.1e-4  6.6e-5  3.5e-4  2.2e-5  1.3e-4  7.0e-5  2.0e-5
#   fp16x2  1.3e-3  5.0e-6  1.9e-3  2.6e-5  1.1e-3  5.3e-6  2.2e-3  1.1e-3
#   fp16    1.6e-3  7.0e-3  3.1e-3  2.5e-3  1.1e-3  9.1e-3  4.1e-3  1.1e-3
#   bf16    1.2e-2  5.6e-2  2.8e-2  2.2e-2  8.8e-3  6.5e-2  3.4e-2  9.0e-3
# Where 3x would pass a ceiling the bound IS the ceiling: the 3-term attention of the stress case (fp16x3 2.6e-5, bf16x3 3.5e-4:
# the peaked softmax of qk = 5 turns the split's score error into probability error) and bf16's LayerNorm planes (one bf16
# rounding: ~2^-9 of an outlier channel at ~30x the row RMS, ~0.06).  The worst rows are scattered over sequences, tokens and 256-row tile positions.
STAGE_BOUND = {
    "fp16x3": dict(embed=2e-5, ln1=2e-5, qkv=2.5e-5, attn=5e-5, x_attn=2e-5, ln2=1.5e-5, fc1=4e-5, x_mlp=2.5e-5),
    "bf16x3": dict(embed=1e-4, ln1=3e-4, qkv=2e-4, attn=5e-4, x_attn=6e-5, ln2=4e-4, fc1=2e-4, x_mlp=6e-5),
    "fp16x2": dict(embed=4e-3, ln1=2e-5, qkv=5e-3, attn=8e-5, x_attn=3.5e-3, ln2=2e-5, fc1=5e-3, x_mlp=3.5e-3),
    "fp16": dict(embed=5e-3, ln1=2e-2, qkv=1e-2, attn=8e-3, x_attn=3.5e-3, ln2=2e-2, fc1=1.2e-2, x_mlp=3.5e-3),
    "bf16": dict(embed=4e-2, ln1=1e-1, qkv=8e-2, attn=7e-2, x_attn=3e-2, ln2=1e-1, fc1=1e-1, x_mlp=3e-2),
}
# Score error (helpers.gate_error) of the teacher-forced last layer + final LayerNorm + diff + head, both last-layer paths.  Ceilings:
# fp16x3 1e-4, bf16x3 3e-4, the other modes their TOL of tests/test_gpu_parity.py.  Observed, worst of the cases that run the mode
# (profiles/r08_stage_parity.txt): fp16x3 3.1e-6, bf16x3 2.7e-5, fp16x2 1.1e-4, fp16 1.2e-3, bf16 1.9e-3.
TAIL_BOUND = {"fp16x3": 1e-5, "bf16x3": 8e-5, "fp16x2": 4e-4, "fp16": 4e-3, "bf16": 6e-3}


# ---- cases -------------------------------------------------------------------------------------------------------------

def _own_case(kw, B, N, wseed, iseed, stress=None):
    kw = json.loads(json.dumps(kw))
    kw["vit_config"]["pretrained"] = False
    spec = make_spec(**json.loads(json.dumps(kw)))
    sd = stress_state(spec, wseed, **stress) if stress else synth.make_state_dict(spec, wseed)
    return kw, spec, sd, synth.make_inputs(spec, B, N, iseed), B, N


def _golden_case(name):
    g, kw, spec, sd, inputs = load_case(name)
    return kw, spec, sd, inputs, int(g["B"]), int(g["N"])


CASES = {
    # name: (build, modes, token_num of the tail check)
    "c2_b32_n500": (lambda: _golden_case("c2_b32_n500"), ALL_MODES, 0),
    # stress5h_b64_n500's weights (the operating-point ladder's), 32 pairs of flat inputs
    "stress5h_b32_n500": (lambda: _own_case(dict(vit_config=dict(variant="ViT-B16")), 32, 500, 32, 61, dict(qk=5.0, head=True)), ALL_MODES, 0),
    # c2shape_b4_n500's kwargs, three layers
    "c2shape_b2_n500": (lambda: _own_case(dict(vit_config=dict(variant="ViT-B16", num_keep_layers=3)), 2, 500, 5, 15), ALL_MODES, 0),
    "refdefault_b16_n512": (lambda: _golden_case("refdefault_b16_n512"), ["fp16x3", "bf16x3", "fp16"], 5),
    # c4_vitl_b16_n1024's kwargs and weights, 4 pairs
    "vitl_b4_n1024": (lambda: _own_case(dict(vit_config=dict(variant="ViT-L16", num_scales=3)), 4, 1024, 53, 63), ["fp16x3", "bf16x3", "fp16"], 0),
    "vitb8_b3_n77": (lambda: _own_case(dict(vit_config=dict(variant="ViT-B8", num_keep_layers=3, num_scales=2, num_extra_tokens=2, num_adapters=1,
                                                        use_layer_scale=True)), 3, 77, 8, 18), ["fp16x3", "bf16x3", "bf16"], 0),
    # the tail check only: 162 sequences, past the switches of launch_skinny's rows-per-workgroup rule at 80 | 81 and 160 | 161 rows
    # (tests/tail_rows.py), through the pair entry and final_diff
    # (stress5h_b32_n500's weights: the head at its operating point -- a random head's scores of 8-patch images are cancellation remainders)
    "vitb_b81_n8": (lambda: _own_case(dict(vit_config=dict(variant="ViT-B16")), 81, 8, 32, 19, dict(qk=5.0, head=True)), ALL_MODES, 0),
}
STAGE_CASES = ["c2_b32_n500", "stress5h_b32_n500", "c2shape_b2_n500", "refdefault_b16_n512", "vitl_b4_n1024", "vitb8_b3_n77"]
TAIL_CASES = ["stress5h_b32_n500", "refdefault_b16_n512", "vitl_b4_n1024", "vitb_b81_n8"]

_cache = {}


def get_case(name):
    """One case at a time (the parametrisations below keep a case's tests together): host weights, fp64 GPU weights, inputs."""
    if name not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        kw, spec, sd, (patches, pos, scales), B, N = CASES[name][0]()
        _cache[name] = dict(kw=kw, spec=spec, sd=sd, sdr=RefWeights(sd), B=B, N=N, patches=patches, pos=pos, scales=scales)
    return _cache[name]


def build(c, precision, options=0, token_num=0):
    m = VTAMIQ(**json.loads(json.dumps(c["kw"])), precision=precision, engine_options=options)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()}, strict=True)
    m = m.to(DEV).eval()
    m.token_num = token_num
    return m


def checked_layers(L):
    return sorted({0, L // 2, L - 2} & set(range(L - 1)))


# ---- fp64 references ---------------------------------------------------------------------------------------------------

def _lin(a, sdr, name):
    return a @ sdr[name + ".weight"].t() + sdr[name + ".bias"]


def qkv_weights(sdr, pre, q_log2):
    s = Q_LOG2_SCALE if q_log2 else 1.0
    w = torch.cat([sdr[pre + "attn.query.weight"] * s, sdr[pre + "attn.key.weight"], sdr[pre + "attn.value.weight"]])
    b = torch.cat([sdr[pre + "attn.query.bias"] * s, sdr[pre + "attn.key.bias"], sdr[pre + "attn.value.bias"]])
    return w, b


def attention_ref(qkv, nh, q_log2):
    """softmax(Q K^T * scale) V per sequence and head from the engine's QKV rows [nseq, S, 3H]; Q in log2 units for the 3-term modes."""
    nseq, S, H3 = qkv.shape
    H = H3 // 3
    dh = H // nh
    scale = math.log(2.0) if q_log2 else 1.0 / math.sqrt(dh)
    out = torch.empty(nseq, S, H, dtype=torch.float64, device=qkv.device)
    step = max(1, (1 << 26) // (nh * S * S))                        # <= 512 MiB of fp64 scores at a time
    for s0 in range(0, nseq, step):
        q, k, v = (t.reshape(-1, S, nh, dh).transpose(1, 2) for t in qkv[s0:s0 + step].split(H, -1))
        p = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
        out[s0:s0 + step] = (p @ v).transpose(1, 2).reshape(-1, S, H)
    return out


def branch(sdr, spec, pre, h, site):
    """A branch output h -> (adapter pair 0, site 1 / 2) -> LayerScale: what the residual GEMM (+ adapter GEMMs) adds to x."""
    if spec.num_adapters > 0:
        h = O.adapter(sdr, f"{pre}adapter{site}.", h)
    if spec.use_layer_scale:
        h = h * sdr[f"{pre}ls{site}.gamma"]
    return h


def embeddings_ref(c, spec):
    sdr = c["sdr"]
    p, ps, sc = split_inputs(c["patches"], c["pos"], c["scales"], device=DEV)
    # patches in fp64; positions and scales stay fp32: the table index is floor(pos * G) in the input's dtype (oracle.pos_index)
    return torch.cat([O.embeddings(sdr, spec, p[i].double(), ps[i], sc[i]) for i in range(2)])


# ---- the stage walk ----------------------------------------------------------------------------------------------------

def stage_walk(pr, sdr, layers, bounds, tag, embed_ref=None) -> StageLog:
    """Grab every stage of `layers` (and the embedding when embed_ref is given), compare each with its fp64 reference row by row and
    check the pad rows behind the last sequence after every stage."""
    spec, H, Md, nh = pr.spec, pr.H, pr.Md, pr.spec.num_heads
    q_log2 = pr.mode in THREE_TERM_ATTENTION
    log = StageLog(tag)

    def pads(layer, stage, st):
        bad = pr.pad_rows_finite(st)
        if bad:
            log.fail(layer, stage + " pad rows", f"non-finite pad rows in {bad}")

    if embed_ref is not None:
        st = pr.grab(0, 0)
        log.check(-1, "embed", pr.x(st), embed_ref, bounds["embed"])
        pads(0, "embed", st)
    for layer in layers:
        pre = f"transformer.encoder.layers.{layer}."
        st = [None] * 7
        for k in range(7):
            st[k] = pr.grab(layer, k)
            pads(layer, STAGES[k], st[k])
        x_in, x_attn = pr.x(st[0]).double(), pr.x(st[3]).double()
        ln1, attn, ln2 = pr.ln(st[0]), pr.ln(st[2]), pr.ln(st[4])
        qkv, fc1 = pr.big(st[1], 3 * H), pr.big(st[5], Md)
        log.check(layer, "ln1", ln1, O._layer_norm(x_in, sdr[pre + "attention_norm.weight"], sdr[pre + "attention_norm.bias"]), bounds["ln1"])
        w, b = qkv_weights(sdr, pre, q_log2)
        log.check(layer, "qkv", qkv, ln1 @ w.t() + b, bounds["qkv"])
        log.check(layer, "attn", attn, attention_ref(qkv, nh, q_log2), bounds["attn"])
        log.check(layer, "x_attn", pr.x(st[3]), x_in + branch(sdr, spec, pre, _lin(attn, sdr, pre + "attn.out"), 1), bounds["x_attn"])
        log.check(layer, "ln2", ln2, O._layer_norm(x_attn, sdr[pre + "ffn_norm.weight"], sdr[pre + "ffn_norm.bias"]), bounds["ln2"])
        log.check(layer, "fc1", fc1, Fn.gelu(_lin(ln2, sdr, pre + "ffn.fc1")), bounds["fc1"])
        log.check(layer, "x_mlp", pr.x(st[6]), x_attn + branch(sdr, spec, pre, _lin(fc1, sdr, pre + "ffn.fc2"), 2), bounds["x_mlp"])
        del st, x_in, x_attn, ln1, attn, ln2, qkv, fc1
    return log


def _case_params(names, with_options=False):
    out = []
    for n in names:
        for mode in CASES[n][1]:
            if with_options:
                out += [pytest.param(n, mode, o, id=f"{n}-{mode}-{'full' if o else 'pruned'}") for o in (0, _lib.OPT_FULL_LAST_LAYER)]
            else:
                out.append(pytest.param(n, mode, id=f"{n}-{mode}"))
    return out


@pytest.mark.parametrize("name,mode", _case_params(STAGE_CASES))
def test_stages_teacher_forced(name, mode):
    c = get_case(name)
    spec, B, N = c["spec"], c["B"], c["N"]
    model = build(c, mode)
    args = split_inputs(c["patches"], c["pos"], c["scales"], device=DEV)
    pr = StageProbe(model, args, B, N)
    layers = checked_layers(spec.num_layers)
    print(f"\n[{name} {mode}] nseq {pr.nseq} x S {pr.S} = {pr.nseq * pr.S} rows (M_pad {pr.M_pad}), layers {layers}")
    stage_walk(pr, c["sdr"], layers, STAGE_BOUND[mode], f"{name} {mode}", embed_ref=embeddings_ref(c, spec)).assert_ok()


# ---- the CLS-only last layer and the head ------------------------------------------------------------------------------

def tail_rows_ref(sdr, spec, x, t, hidden=False):
    """The residual rows xr [nseq, H] of token t behind the last layer, before encoder_norm, from the stream x [nseq, S, H] entering that
    layer: LayerNorm 1, the token's query against keys and values of every row, out-proj, LayerNorm 2 and the MLP, in fp64.  These are the
    rows encode_reference() exports (tests/test_gpu_tail_rows.py).  hidden=True: (xr, the fc1 + GELU rows [nseq, mlp_dim] fc2 consumes)."""
    L, nh = spec.num_layers, spec.num_heads
    pre = f"transformer.encoder.layers.{L - 1}."
    nseq, S, H = x.shape
    dh = H // nh
    ln = O._layer_norm(x, sdr[pre + "attention_norm.weight"], sdr[pre + "attention_norm.bias"])
    q = _lin(ln[:, t], sdr, pre + "attn.query").view(nseq, nh, 1, dh)
    k = _lin(ln, sdr, pre + "attn.key").view(nseq, S, nh, dh).transpose(1, 2)
    v = _lin(ln, sdr, pre + "attn.value").view(nseq, S, nh, dh).transpose(1, 2)
    ctx = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), -1) @ v).reshape(nseq, H)
    xa = x[:, t] + branch(sdr, spec, pre, _lin(ctx, sdr, pre + "attn.out"), 1)
    h = Fn.gelu(_lin(O._layer_norm(xa, sdr[pre + "ffn_norm.weight"], sdr[pre + "ffn_norm.bias"]), sdr, pre + "ffn.fc1"))      # O.mlp, in its two halves
    xr = xa + branch(sdr, spec, pre, _lin(h, sdr, pre + "ffn.fc2"), 2)
    return (xr, h) if hidden else xr


def tail_scores(sdr, spec, xr, B):
    """Scores of B pairs from their 2B rows xr behind the last layer (references first): encoder_norm, ref - dist, the head, in fp64."""
    y = O._layer_norm(xr, sdr["transformer.encoder.encoder_norm.weight"], sdr["transformer.encoder.encoder_norm.bias"])
    return O.head(sdr, spec, y[:B, None], y[B:, None], 0)


def tail_ref(sdr, spec, x, B, t, rows=False):
    """Scores from the stream x [2B, S, H] entering the last layer: that layer's token-t rows (K / V from every row), encoder_norm, the
    ref - dist difference and the head, in fp64.  rows=True: (scores, the rows xr before encoder_norm)."""
    xr = tail_rows_ref(sdr, spec, x, t)
    q = tail_scores(sdr, spec, xr, B)
    return (q, xr) if rows else q


@pytest.mark.parametrize("name,mode,options", _case_params(TAIL_CASES, with_options=True))
def test_cls_tail_teacher_forced(name, mode, options):
    """cls_tail.hip (pruned) and the full last layer (VTQ_OPT_FULL_LAST_LAYER), final_diff_kernel and the skinny head at production size,
    against fp64 from the engine's own stream entering the last layer: both last-layer paths meet one bound."""
    c = get_case(name)
    spec, B, N, t = c["spec"], c["B"], c["N"], CASES[name][2]
    L = spec.num_layers
    model = build(c, mode, options, token_num=t)
    args = split_inputs(c["patches"], c["pos"], c["scales"], device=DEV)
    pr = StageProbe(model, args, B, N)
    x = pr.x(pr.grab_stop((L - 2) * 7 + 6 if L > 1 else 0, want=("x",))).double()
    with torch.no_grad():
        q = model(*args)[0].cpu().numpy()                  # one normal forward: the same bits up to the last layer (deterministic)
    q_ref = tail_ref(c["sdr"], spec, x, B, t).cpu().numpy()
    e = gate_error(q, q_ref)
    print(f"\n[{name} {mode} {'full last layer' if options else 'CLS-only tail'}] token {t}: scores {q_ref.min():.3g} .. {q_ref.max():.3g}, "
          f"gate error {e:.2e}   bound {TAIL_BOUND[mode]:.2g}")
    assert np.isfinite(q).all() and e <= TAIL_BOUND[mode], (e, TAIL_BOUND[mode])


# ---- the check can fail ------------------------------------------------------------------------------------------------

def test_stage_check_flags_a_perturbed_fc2_weight():
    """One element of layer 1's fc2 weight moved in the fp64 reference's copy, by an amount that puts the worst affected row at about 8x
    the fp16x3 bound while the fp64 scores move by less than any score-level gate resolves: the stage walk fails at exactly (layer 1, x_mlp)."""
    name, mode, layer = "c2shape_b2_n500", "fp16x3", 1
    c = get_case(name)
    spec, B, N = c["spec"], c["B"], c["N"]
    model = build(c, mode)
    args = split_inputs(c["patches"], c["pos"], c["scales"], device=DEV)
    pr = StageProbe(model, args, B, N)
    bounds = STAGE_BOUND[mode]
    g = pr.big(pr.grab(layer, 5), spec.mlp_dim)                    # the fc1 + GELU rows fc2 consumes
    x = pr.x(pr.grab(layer, 3)).double()                           # the residual x_mlp is measured against
    j = int(g.abs().amax((0, 1)).argmax())                         # the hidden unit with the largest activation
    reach = g[..., j].abs() / x.pow(2).mean(-1).sqrt()             # what a unit change of W2[:, j] does to each row, relative to its RMS
    s, r = divmod(int(reach.argmax()), pr.S)
    ch = 5
    delta = 8.0 * bounds["x_mlp"] / float(reach[s, r])
    key = f"transformer.encoder.layers.{layer}.ffn.fc2.weight"
    sd2 = dict(c["sd"])
    sd2[key] = c["sd"][key].copy()
    sd2[key][ch, j] += delta
    sdr2 = RefWeights(sd2)
    print(f"\n[{name} {mode}] {key}[{ch}, {j}] += {delta:.3e} (weight rms {float(np.sqrt(np.mean(c['sd'][key] ** 2))):.3e})")
    over = stage_walk(pr, sdr2, checked_layers(spec.num_layers), bounds, "perturbed").over()
    assert [(l, st) for l, st, *_ in over] == [(layer, "x_mlp")], over
    assert over[0][3][:2] == (s, r), over                           # ... and it names the row the perturbation hit hardest
    # the same perturbation end to end: the fp64 model's scores move by less than the fp16x3 tail bound (1e-5, a hundredth of the 1e-3 claim)
    p, ps, sc = split_inputs(c["patches"], c["pos"], c["scales"], device=DEV)
    p = tuple(t.double() for t in p)
    q0 = O.vtamiq_forward(c["sdr"], spec, p, ps, sc)[0].cpu().numpy()
    q1 = O.vtamiq_forward(sdr2, spec, p, ps, sc)[0].cpu().numpy()
    e = gate_error(q1, q0)
    print(f"   fp64 scores with the perturbed weight: gate error {e:.2e} against the unperturbed model")
    assert e < TAIL_BOUND[mode], e
