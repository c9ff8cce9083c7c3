"""Attention rollout through the variable-length, group and cached entries on the MI355X: forward_rollout(lengths=), forward_group /
encode_reference / forward_cached (rollout=True, with and without lengths=), and the table-driven step kernel behind them
(vtq_vl_rollout_step, include/vtamiq_hip_rollout.h).

Every check is an equality of bits.  The reference is never the code under test: the table-driven kernel is compared with the uniform kernel
(vtq_k_rollout_step) on one sequence alone, the new entries with forward_rollout on a single pair (B = 1) and with the score-only entries
(forward_varlen, forward_group, encode_reference, forward_cached).  The uniform entry itself is pinned against fp64 in
tests/test_gpu_rollout.py; the only bound used here is that file's: a rollout vector sums to 1 within 1e-5 in the 3-term modes.

A sequence's maps depend on its own image alone, so where a reference and a distorted image have different patch counts the single pair that
holds an image pairs it with itself.

All models: ViT-B/16, num_keep_layers=2 (the r = e_token first step behind the last layer's Q | K projection, and a second step on r),
synthetic seeded weights with peaked attention (tests/helpers.py stress_state) and a small head."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests.footprint import Arena
from tests.gpu_util import stream, to_planes
from tests.helpers import stress_state
from tests.interleave import bits, same_bits
from tests.test_gpu_forward_vit import THREE_TERM_ATTENTION
from vtamiq_amd import VTAMIQ, Rollout, _lib, synth
from vtamiq_amd.spec import make_spec

pytestmark = pytest.mark.gpu

DEV = "cuda"
FULL = _lib.OPT_FULL_LAST_LAYER
KW = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False), num_rgs=2, num_rcabs=2, ca_reduction=16)
KW_REG = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_extra_tokens=8, pretrained=False), num_rgs=2, num_rcabs=2, ca_reduction=16)
# (precision, engine options): fp16x3 with the CLS-only last layer and with the full one, one case each in fp16 and bf16x3
CONFIGS = [("fp16x3", 0), ("fp16x3", FULL), ("fp16", 0), ("bf16x3", 0)]
CONFIG_IDS = ["fp16x3", "fp16x3-full-last-layer", "fp16", "bf16x3"]
H, NH = 768, 12

_cache = {}


def spec_of(kw):
    return make_spec(**json.loads(json.dumps(kw)))


def model(precision, options=0, kw=KW, token=0):
    key = ("sd", json.dumps(kw, sort_keys=True))
    if key not in _cache:
        _cache[key] = stress_state(spec_of(kw), 71, qk=4.0)
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision=precision, engine_options=options)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _cache[key].items()})
    m.token_num = token
    m.validate_inputs = False
    return m.to(DEV).eval()


def images(lengths, seed, kw=KW):
    """Per image i a (ref, dist) pair of lengths[i] patches: ([ref_i], [dist_i], [pos_i]) lists of device tensors, seeded, made once."""
    key = ("img", tuple(lengths), seed)
    if key not in _cache:
        pa, po, _ = synth.make_inputs(spec_of(kw), 1, sum(lengths), seed)
        cut = np.cumsum([0] + list(lengths))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        _cache[key] = tuple([dev(a[cut[i]:cut[i + 1]]) for i in range(len(lengths))] for a in (pa[0, 0], pa[0, 1], po[0, 0]))
    return _cache[key]


def single_pair(m, p_ref, p_dist, pos_ref, pos_dist):
    """forward_rollout on ONE pair: (q (1,), rollout (2, S), last_attention (2, h, S))."""
    with torch.no_grad():
        q, r = m.forward_rollout((p_ref[None], p_dist[None]), (pos_ref[None], pos_dist[None]), None)
    return q, r.rollout[:, 0], r.last_attention[:, 0]


def assert_positive_and_normalised(precision, maps, heads):
    for v, a in zip(maps, heads):
        assert torch.isfinite(v).all() and float(v.min()) > 0 and float(a.min()) > 0
        if precision in THREE_TERM_ATTENTION:
            assert abs(float(v.double().sum()) - 1.0) <= 1e-5          # the bound of tests/test_gpu_rollout.py check()


# ==== kernel level: vtq_vl_rollout_step =======================================================================================================
# every seam: the 32-row wave, the 64-key tile, the 128-row query block, 2 and 3 blocks; short and long sequences alternate
SEQ = [300, 2, 257, 31, 256, 32, 193, 33, 129, 64, 128, 65, 127]
assert sorted(SEQ) == [2, 31, 32, 33, 64, 65, 127, 128, 129, 193, 256, 257, 300]
ROW0 = [int(v) for v in np.cumsum([0] + SEQ[:-1])]
R = sum(SEQ)
NQB_MAX = (max(SEQ) + 127) // 128
STEP_FORMATS = [("fp16x3", 1), ("fp16", 0), ("bf16x3", 1)]          # (operand format, q_log2)


def step_inputs(fmt):
    """(fp32 qkv rows (R, 3H) with Q pre-scaled for the 3-term formats, r_in (R,): positive, each sequence summing to 1).  Seeded; clones only."""
    key = ("step", fmt)
    if key not in _cache:
        g = torch.Generator(device="cpu").manual_seed(11)
        qkv = torch.randn(R, 3 * H, generator=g) * 0.5
        if fmt.endswith("x3"):
            qkv[:, :H] *= 0.125 * math.log2(math.e)
        r = torch.rand(R, generator=g) + 0.05
        for o, S in zip(ROW0, SEQ):
            r[o:o + S] /= r[o:o + S].sum()
        _cache[key] = (qkv.to(DEV), r.float().to(DEV))
    return _cache[key]


def vl_step(planes, r_in, r_out, part, fmt, q_log2):
    lens = (C.c_int32 * len(SEQ))(*SEQ)
    _lib.check(_lib.load().vtq_vl_rollout_step(planes.data_ptr(), planes[0].numel(), r_in.data_ptr(), r_out.data_ptr(), part.data_ptr(), len(SEQ), lens,
                                               H, _lib.NUM[fmt], q_log2, stream()))


def vl_step_clean(fmt, q_log2):
    key = ("step out", fmt)
    if key not in _cache:
        qkv, r = step_inputs(fmt)
        out = torch.full((R,), float("nan"), device=DEV)
        part = torch.full((NH * NQB_MAX * R,), float("nan"), device=DEV)
        vl_step(to_planes(qkv, fmt), r, out, part, fmt, q_log2)
        torch.cuda.synchronize()
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("fmt,q_log2", STEP_FORMATS, ids=[f for f, _ in STEP_FORMATS])
def test_step_on_packed_sequences_has_the_bits_of_the_uniform_kernel_on_each_alone(fmt, q_log2):
    lib = _lib.load()
    qkv, r = step_inputs(fmt)
    planes = to_planes(qkv, fmt)
    got = vl_step_clean(fmt, q_log2)
    assert torch.isfinite(got).all() and float(got.min()) > 0
    for o, S in zip(ROW0, SEQ):
        alone = planes[:, o:o + S].contiguous()                               # the sequence's own rows and nothing else
        r_j = r[o:o + S].contiguous()
        out = torch.full((S,), float("nan"), device=DEV)
        part = torch.full((NH * ((S + 127) // 128) * S,), float("nan"), device=DEV)
        _lib.check(lib.vtq_k_rollout_step(alone.data_ptr(), alone[0].numel(), r_j.data_ptr(), out.data_ptr(), part.data_ptr(), 1, S, S, H,
                                          _lib.NUM[fmt], q_log2, stream()))
        torch.cuda.synchronize()
        assert same_bits(got[o:o + S], out), f"S = {S}: {int((bits(got[o:o + S]) != bits(out)).sum())} of {S} values differ"
        assert abs(float(out.double().sum()) - 1.0) <= 1e-5                    # r sums to 1 and every P row does


@pytest.mark.parametrize("poison", [float("nan"), 6e4], ids=["nan", "6e4"])
@pytest.mark.parametrize("fmt,q_log2", STEP_FORMATS, ids=[f for f, _ in STEP_FORMATS])
def test_a_sequence_reads_nothing_of_its_neighbours_or_of_the_value_columns(fmt, q_log2, poison):
    qkv, r = step_inputs(fmt)
    clean = vl_step_clean(fmt, q_log2)
    for o, S in zip(ROW0, SEQ):
        bad, bad_r = torch.full_like(qkv, poison), torch.full_like(r, poison)
        bad[o:o + S, :2 * H] = qkv[o:o + S, :2 * H]                              # its own Q and K columns: everything else is poison
        bad_r[o:o + S] = r[o:o + S]
        out = torch.full((R,), float("nan"), device=DEV)
        part = torch.full((NH * NQB_MAX * R,), float("nan"), device=DEV)
        vl_step(to_planes(bad, fmt), bad_r, out, part, fmt, q_log2)
        torch.cuda.synchronize()
        assert same_bits(out[o:o + S], clean[o:o + S]), f"S = {S} at row {o}"


def test_step_outputs_keep_to_the_headers_extents():
    """r_out at exactly R floats and part at exactly (H / 64) * ceil(S_max / 128) * R floats inside guards, both pre-filled with the guard
    byte (part needs no initial value): no guard changes and r_out is the same under both fills."""
    fmt, q_log2 = "fp16x3", 1
    qkv, r = step_inputs(fmt)
    planes = to_planes(qkv, fmt)
    specs = [((R,), torch.float32), ((NH * NQB_MAX * R,), torch.float32)]
    a = Arena(fp.arena_bytes(specs), DEV)
    out = a.carve("r_out", (R,), torch.float32)
    part = a.carve("part", (NH * NQB_MAX * R,), torch.float32)
    fills = iter((0x00, 0xFF))

    def prepare():
        byte = next(fills)
        a.fill(out, byte)
        a.fill(part, byte)
    got, = a.run_twice(lambda: vl_step(planes, r, out, part, fmt, q_log2), lambda: [out], prepare=prepare)
    assert same_bits(got, vl_step_clean(fmt, q_log2))


# ==== end to end ==============================================================================================================================
LENS = [1, 31, 63, 127, 128, 200]               # S = N + 1 = 2, 32, 64, 128, 129, 201: on and next to the wave, tile and block seams


def ragged_call(m, lengths=LENS, seed=81, kw=KW):
    pr, pd, po = images(lengths, seed, kw)
    with torch.no_grad():
        return m.forward_rollout((pr, pd), (po, po), None, lengths=lengths)


def flat(r: Rollout):
    """A ragged Rollout's tensors in a fixed order (for comparisons of whole calls)."""
    out = []
    for side in (0, 1):
        out += list(r.rollout[side]) + list(r.last_attention[side])
    return out


@pytest.mark.parametrize("precision,options", CONFIGS, ids=CONFIG_IDS)
def test_forward_rollout_with_lengths(precision, options):
    m = model(precision, options)
    pr, pd, po = images(LENS, 81)
    q, got = ragged_call(m)
    with torch.no_grad():
        q0, none = m.forward_varlen((pr, pd), (po, po), None, LENS)
    assert none is None and same_bits(q, q0), "q differs from forward_varlen"
    assert isinstance(got, Rollout) and Rollout._fields == ("rollout", "last_attention")
    T = m.spec.num_tokens
    base = [got.rollout[0][0].untyped_storage().data_ptr(), got.last_attention[0][0].untyped_storage().data_ptr()]
    for b, n in enumerate(LENS):
        qb, roll, last = single_pair(m, pr[b], pd[b], po[b], po[b])
        assert same_bits(q[b:b + 1], qb), b
        for side in (0, 1):
            v, a = got.rollout[side][b], got.last_attention[side][b]
            assert v.shape == (n + T,) and a.shape == (NH, n + T)
            assert [v.untyped_storage().data_ptr(), a.untyped_storage().data_ptr()] == base, "not a view of the call's flat allocation"
            assert same_bits(v, roll[side]), (b, side, "rollout")
            assert same_bits(a, last[side]), (b, side, "last_attention")
    for side in (0, 1):
        assert_positive_and_normalised(precision, got.rollout[side], got.last_attention[side])


@pytest.mark.parametrize("precision,options", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_equal_lengths_give_the_bits_of_the_uniform_entry(precision, options):
    m = model(precision, options)
    lens = [40, 40, 40]
    pr, pd, po = images(lens, 82)
    with torch.no_grad():
        q, got = m.forward_rollout((pr, pd), (po, po), None, lengths=lens)
        q0, want = m.forward_rollout((torch.stack(pr), torch.stack(pd)), (torch.stack(po), torch.stack(po)), None)
    assert same_bits(q, q0)
    for side in (0, 1):
        assert same_bits(torch.stack(got.rollout[side]), want.rollout[side])
        assert same_bits(torch.stack(got.last_attention[side]), want.last_attention[side])


# ---- one-to-many ----------------------------------------------------------------------------------------------------------------------------
G, M, N, INDEX = 2, 5, 40, [1, 0, 1, 1, 0]
LENS_REF, LENS_DIST = [33, 129], [1, 64, 200, 127, 5]


def group_inputs(ragged):
    """(p_ref, p_dist, pos_ref, pos_dist) as lists of per-image tensors: G references, M distorted images of reference INDEX[m]."""
    if not ragged:
        pr, pd, po = images([N] * G, 83)
        _, pd2, po2 = images([N] * M, 84)
        return pr, pd2, po, po2
    pr, _, po = images(LENS_REF, 85)
    _, pd, po2 = images(LENS_DIST, 86)
    return pr, pd, po, po2


def group_call(m, ragged, rollout=True, inp=None):
    pr, pd, qr, qd = inp if inp is not None else group_inputs(ragged)
    with torch.no_grad():
        if ragged:
            return m.forward_group((pr, pd), (qr, qd), None, INDEX, lengths=(LENS_REF, LENS_DIST), rollout=rollout)
        return m.forward_group((torch.stack(pr), torch.stack(pd)), (torch.stack(qr), torch.stack(qd)), None, INDEX, rollout=rollout)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "lengths"])
@pytest.mark.parametrize("precision,options", CONFIGS, ids=CONFIG_IDS)
def test_forward_group_with_rollout(precision, options, ragged):
    m = model(precision, options)
    pr, pd, qr, qd = group_inputs(ragged)
    q, got = group_call(m, ragged)
    q0, none = group_call(m, ragged, rollout=False)
    assert none is None and same_bits(q, q0), "q differs from forward_group"
    (roll_r, roll_d), (last_r, last_d) = got.rollout, got.last_attention
    assert len(roll_r) == len(last_r) == G and len(roll_d) == len(last_d) == M
    if not ragged:
        S = N + m.spec.num_tokens
        assert roll_r.shape == (G, S) and roll_d.shape == (M, S) and last_r.shape == (G, NH, S) and last_d.shape == (M, NH, S)
    seen = set()
    for i in range(M):
        g = INDEX[i]
        if ragged:                                # counts differ inside the pair: each image paired with itself
            _, roll, last = single_pair(m, pd[i], pd[i], qd[i], qd[i])
        else:                                     # the single pair (reference INDEX[i], distorted i): both sides at once
            qi, roll, last = single_pair(m, pr[g], pd[i], qr[g], qd[i])
            assert same_bits(q[i:i + 1], qi), i
            assert same_bits(roll_r[g], roll[0]) and same_bits(last_r[g], last[0]), ("reference", g, "from pair", i)
            seen.add(g)
        assert same_bits(roll_d[i], roll[1]) and same_bits(last_d[i], last[1]), ("distorted", i)
    for g in set(range(G)) - seen:
        _, roll, last = single_pair(m, pr[g], pr[g], qr[g], qr[g])
        assert same_bits(roll_r[g], roll[0]) and same_bits(last_r[g], last[0]), ("reference", g)
    assert_positive_and_normalised(precision, list(roll_r) + list(roll_d), list(last_r) + list(last_d))


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "lengths"])
@pytest.mark.parametrize("precision,options", CONFIGS, ids=CONFIG_IDS)
def test_encode_reference_and_forward_cached_with_rollout(precision, options, ragged):
    m = model(precision, options)
    pr, pd, qr, qd = group_inputs(ragged)
    q_group, want = group_call(m, ragged)
    cat = (lambda ts: torch.cat(ts)) if ragged else (lambda ts: torch.stack(ts))
    kr = dict(lengths=LENS_REF) if ragged else {}
    kd = dict(lengths=LENS_DIST) if ragged else {}
    with torch.no_grad():
        ref, maps_r = m.encode_reference(cat(pr), cat(qr), None, rollout=True, **kr)
        ref0 = m.encode_reference(cat(pr), cat(qr), None, **kr)
        q, maps_d = m.forward_cached(ref, cat(pd), cat(qd), None, INDEX, rollout=True, **kd)
        q0, none = m.forward_cached(ref0, cat(pd), cat(qd), None, INDEX, **kd)
    assert same_bits(ref.rows, ref0.rows), "the cached rows differ from encode_reference's"
    assert none is None and same_bits(q, q0) and same_bits(q, q_group)
    assert isinstance(maps_r, Rollout) and isinstance(maps_d, Rollout)
    for got, side, n in ((maps_r, 0, G), (maps_d, 1, M)):
        assert len(got.rollout) == len(got.last_attention) == n
        for i in range(n):
            assert same_bits(got.rollout[i], want.rollout[side][i]), (side, i, "rollout")
            assert same_bits(got.last_attention[i], want.last_attention[side][i]), (side, i, "last_attention")


def test_register_token():
    """num_extra_tokens = 8, token_num = 3: the walk starts at token 3 and last_attention is row 3 of the last layer's maps."""
    lens = [5, 130, 63]
    m = model("fp16x3", kw=KW_REG, token=3)
    pr, pd, po = images(lens, 87, KW_REG)
    q, got = ragged_call(m, lens, 87, KW_REG)
    T = m.spec.num_tokens
    assert T == 9
    for b in range(len(lens)):
        _, roll, last = single_pair(m, pr[b], pd[b], po[b], po[b])
        for side in (0, 1):
            assert same_bits(got.rollout[side][b], roll[side]) and same_bits(got.last_attention[side][b], last[side]), (b, side)
    enc = m.transformer.encoder
    enc.return_attention = True
    with torch.no_grad():
        _, maps, _ = m.forward_vit(pr[1][None], po[1][None], None, tokens_only=True)
    enc.return_attention = False
    assert same_bits(got.last_attention[0][1], maps[-1][0, :, 3, :]), "last_attention is not row 3 of forward_vit's last map"
    m.token_num = 0
    _, cls = ragged_call(m, lens, 87, KW_REG)
    assert float((cls.rollout[0][1] - got.rollout[0][1]).abs().max()) > 1e-4      # the token matters


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "lengths"])
def test_a_nan_image_reaches_its_own_score_and_maps_only(ragged):
    m = model("fp16x3")
    inp = group_inputs(ragged)
    q, clean = group_call(m, ragged)

    def poisoned(which, i):
        out = [list(t) for t in inp]
        t = out[which][i].clone()
        t[0, 1, 3, 3] = float("nan")
        out[which][i] = t
        return out

    # distorted image 2
    qn, got = group_call(m, ragged, inp=poisoned(1, 2))
    assert torch.isnan(qn[2]) and same_bits(torch.cat([qn[:2], qn[3:]]), torch.cat([q[:2], q[3:]]))
    assert torch.isnan(got.rollout[1][2]).all() and torch.isnan(got.last_attention[1][2]).all()
    for g in range(G):
        assert same_bits(got.rollout[0][g], clean.rollout[0][g]) and same_bits(got.last_attention[0][g], clean.last_attention[0][g])
    for i in (0, 1, 3, 4):
        assert same_bits(got.rollout[1][i], clean.rollout[1][i]) and same_bits(got.last_attention[1][i], clean.last_attention[1][i])
    # reference 1: its own maps and the scores pointing at it
    qn, got = group_call(m, ragged, inp=poisoned(0, 1))
    hit = torch.tensor([g == 1 for g in INDEX], device=DEV)
    assert torch.equal(torch.isnan(qn), hit) and same_bits(qn[~hit], q[~hit])
    assert torch.isnan(got.rollout[0][1]).all() and torch.isnan(got.last_attention[0][1]).all()
    assert same_bits(got.rollout[0][0], clean.rollout[0][0]) and same_bits(got.last_attention[0][0], clean.last_attention[0][0])
    for i in range(M):
        assert same_bits(got.rollout[1][i], clean.rollout[1][i]) and same_bits(got.last_attention[1][i], clean.last_attention[1][i])


# ---- one engine, several calls, no host synchronisation between them --------------------------------------------------------------------------
def uniform_large(m, scale=1.0):
    pr, pd, po = images([300] * 3, 88)
    with torch.no_grad():
        q, r = m.forward_rollout((torch.stack(pr) * scale, torch.stack(pd) * scale), (torch.stack(po), torch.stack(po)), None)
    return [q, r.rollout, r.last_attention]


def fresh(what):
    """The call on an engine that runs nothing else: computed once, never modified."""
    key = ("fresh", what)
    if key not in _cache:
        torch.cuda.synchronize()
        m = model("fp16x3")
        if what == "ragged":
            q, r = ragged_call(m)
            out = [q] + flat(r)
        else:
            out = uniform_large(m)
        torch.cuda.synchronize()
        _cache[key] = [t.clone() for t in out]
    return _cache[key]


def assert_same_call(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), f"{what}: output {k} differs from the fresh engine's"


def test_large_uniform_then_ragged_then_uniform_on_one_engine():
    want_u, want_r = fresh("uniform"), fresh("ragged")
    torch.cuda.synchronize()
    m = model("fp16x3")
    first = uniform_large(m)
    q, r = ragged_call(m)
    again = uniform_large(m)
    torch.cuda.synchronize()
    assert_same_call(first, want_u, "uniform, first")
    assert_same_call([q] + flat(r), want_r, "ragged behind the large uniform call")
    assert_same_call(again, want_u, "uniform behind the ragged call")


def test_ragged_rollout_behind_a_call_that_overflowed_fp16():
    """Patches of 1e8 leave the fp16 operand range: the retained QKV buffers hold inf / NaN up to the large call's rows, far behind the small
    ragged call's M_pad.  precision is "fp16x3", not "auto": nothing repeats the call or reads the error word in between."""
    want = fresh("ragged")
    torch.cuda.synchronize()
    m = model("fp16x3")
    bad = uniform_large(m, scale=1e8)
    q, r = ragged_call(m)
    torch.cuda.synchronize()
    assert not torch.isfinite(bad[0]).any(), "the carrier call did not overflow"
    assert_same_call([q] + flat(r), want, "ragged behind an overflowed call")
    with pytest.raises(FloatingPointError):
        m.check_inputs()                               # the carrier's overflow was recorded, and is cleared by the look


def test_ragged_rollout_behind_a_refused_call():
    want = fresh("ragged")
    torch.cuda.synchronize()
    m = model("fp16x3")
    uniform_large(m)                                   # creates the engine and leaves a larger call's rows and tables behind
    lib, eng = m._engine_lib(), m._engine
    pr, pd, po = images(LENS, 81)
    p0, p1, ps = torch.cat(pr), torch.cat(pd), torch.cat(po)
    qbuf = torch.full((len(LENS),), 7.0, device=DEV)
    roll = torch.full((2 * (sum(LENS) + len(LENS)),), 7.0, device=DEV)
    ok, zero = (C.c_int32 * len(LENS))(*LENS), (C.c_int32 * len(LENS))(*([5, 0] + LENS[2:]))
    args = (eng, p0.data_ptr(), p1.data_ptr(), ps.data_ptr(), ps.data_ptr(), None, None, len(LENS))
    for n_arr, out, text in ((ok, None, b"null rollout_out"), (zero, roll.data_ptr(), b"n_patches[1] = 0")):
        rc = lib.vtq_forward_varlen_rollout(*args, n_arr, qbuf.data_ptr(), out, None, stream())
        assert rc != 0 and b"vtq_forward_varlen_rollout" in lib.vtq_last_error() and text in lib.vtq_last_error(), lib.vtq_last_error()
    q, r = ragged_call(m)
    torch.cuda.synchronize()
    assert bool((qbuf == 7.0).all()) and bool((roll == 7.0).all()), "a refused call wrote an output"
    assert_same_call([q] + flat(r), want, "ragged behind refused calls")


def test_a_token_trace_and_a_debug_stop_are_refused_with_no_launch():
    """What the rollout forms still refuse on a live handle: a set token trace buffer (every variable-length and one-to-many entry does) and a
    set vtq_debug_stop_after (the rollout forms alone).  No output is touched, and the next call has the fresh engine's bits."""
    want = fresh("ragged")
    torch.cuda.synchronize()
    m = model("fp16x3")
    ragged_call(m)                                     # creates the engine
    lib, eng = m._engine_lib(), m._engine
    pr, pd, qr, qd = group_inputs(False)
    p0, p1, s0, s1 = torch.stack(pr), torch.stack(pd), torch.stack(qr), torch.stack(qd)
    S = N + m.spec.num_tokens
    q = torch.full((M,), 7.0, device=DEV)
    roll = torch.full((G + M, S), 7.0, device=DEV)
    rows = torch.full((G, H), 7.0, device=DEV)
    idx = (C.c_int32 * M)(*INDEX)
    trace = torch.zeros(3, G + M, 1, H, device=DEV)

    def calls():
        yield "vtq_forward_group_rollout", lib.vtq_forward_group_rollout(eng, p0.data_ptr(), p1.data_ptr(), s0.data_ptr(), s1.data_ptr(), None, None, G, M,
                                                                         N, idx, q.data_ptr(), roll.data_ptr(), None, stream())
        yield "vtq_encode_reference_rollout", lib.vtq_encode_reference_rollout(eng, p0.data_ptr(), 0, s0.data_ptr(), None, G, N, rows.data_ptr(),
                                                                               roll.data_ptr(), None, stream())
        yield "vtq_forward_cached_rollout", lib.vtq_forward_cached_rollout(eng, rows.data_ptr(), G, p1.data_ptr(), 0, s1.data_ptr(), None, M, N, idx,
                                                                           q.data_ptr(), roll.data_ptr(), None, stream())
    _lib.check(lib.vtq_set_token_trace(eng, trace.data_ptr()))
    try:
        for name, rc in calls():
            assert rc != 0 and name.encode() in lib.vtq_last_error() and b"token trace" in lib.vtq_last_error(), lib.vtq_last_error()
    finally:
        lib.vtq_set_token_trace(eng, None)
    _lib.check(lib.vtq_debug_stop_after(eng, 1))
    try:
        for name, rc in calls():
            assert rc != 0 and name.encode() in lib.vtq_last_error() and b"vtq_debug_stop_after" in lib.vtq_last_error(), lib.vtq_last_error()
    finally:
        lib.vtq_debug_stop_after(eng, -1)
    got_q, r = ragged_call(m)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (q, roll, rows)) and bool((trace == 0).all()), "a refused call wrote an output"
    assert_same_call([got_q] + flat(r), want, "ragged behind refused calls")


def test_ragged_outputs_keep_to_the_headers_extents():
    """vtq_forward_group_varlen_rollout with rollout_out at exactly R and last_attention_out at exactly h * R floats inside guards; a NULL
    last_attention_out is accepted and gives the same rollout."""
    m = model("fp16x3")
    pr, pd, qr, qd = group_inputs(True)
    q_ref, ref = group_call(m, True)
    torch.cuda.synchronize()
    rows = sum(LENS_REF) + sum(LENS_DIST) + (G + M) * m.spec.num_tokens
    specs = [((M,), torch.float32), ((rows,), torch.float32), ((NH * rows,), torch.float32), ((rows,), torch.float32)]
    a = Arena(fp.arena_bytes(specs), DEV)
    q = a.carve("q", (M,), torch.float32)
    roll = a.carve("rollout", (rows,), torch.float32)
    last = a.carve("last_attention", (NH * rows,), torch.float32)
    roll2 = a.carve("rollout (null last_attention)", (rows,), torch.float32)
    lib, eng = m._engine_lib(), m._engine
    p0, p1, s0, s1 = torch.cat(pr), torch.cat(pd), torch.cat(qr), torch.cat(qd)
    nr, nd, idx = (C.c_int32 * G)(*LENS_REF), (C.c_int32 * M)(*LENS_DIST), (C.c_int32 * M)(*INDEX)
    args = (eng, p0.data_ptr(), p1.data_ptr(), s0.data_ptr(), s1.data_ptr(), None, None, G, M, nr, nd, idx, q.data_ptr())

    def launch():
        _lib.check(lib.vtq_forward_group_varlen_rollout(*args, roll.data_ptr(), last.data_ptr(), stream()))
        _lib.check(lib.vtq_forward_group_varlen_rollout(*args, roll2.data_ptr(), None, stream()))
    fills = iter((0x00, 0xFF))

    def prepare():
        byte = next(fills)
        for t in (q, roll, last, roll2):
            a.fill(t, byte)
    gq, gr, gl, gr2 = a.run_twice(launch, lambda: [q, roll, last, roll2], prepare=prepare)
    assert same_bits(gq, q_ref) and same_bits(gr2, gr)
    assert same_bits(gr, torch.cat(list(ref.rollout[0]) + list(ref.rollout[1])))
    assert same_bits(gl, torch.cat([t.reshape(-1) for t in list(ref.last_attention[0]) + list(ref.last_attention[1])]))
