"""Every forward entry interleaved on ONE engine: what a call leaves behind must not reach the next call of any kind.

The catalogue of calls, the plan and the comparison are tests/interleave.py.  Everything is bit for bit (torch.equal on the int32 view);
the reference of a call is the same call on a freshly constructed model that runs nothing else.  That each kind is right on its own is
pinned by its own file (test_gpu_parity, _varlen, _group, _rollout, _forward_vit) and not repeated here.

What of the engine (vtamiq_amd/csrc/engine.hip) or of the model (vtamiq_amd/model.py) each test pins:
  test_any_order                          every ordered pair of kinds, geometries small -> large -> small: stale rows of x / lnbuf / big and of the
                                          rollout buffers ro_qkv behind a smaller call reach no output; no call writes a rollout, layer states or
                                          attention maps it was not asked for; vl_tab shared by varlen's tables and the group / cached ref_index;
                                          returned tensors that alias engine memory
  test_after_a_poisoned_call              stale non-finite rows of x / lnbuf / big and of the ro_qkv buffers behind a smaller call, the error word.
                                          pairwise_small (run first), rollout_small and varlen_small are shaped so that their last 64-key tile reads the
                                          128 slack rows behind M_pad that every forward clears by hand.  The test does NOT tell those
                                          memsets' presence from their absence: with the ro_qkv memset taken out it still passes, because the attention
                                          and rollout-step kernels replace masked scores and zero masked V rows themselves (tests/test_gpu_footprint.py
                                          test_attention pins that for NaN rows).  It pins the outcome -- NaN behind M_pad reaches no output -- not a line
  test_one_poisoned_pair                  masked keys of a NaN neighbour sequence: healthy pairs of the same call keep their bits in every output
  test_after_a_refused_call               a rollout call refused by the shared path's checks, or behind a trace: the calls behind it never write into
                                          the refused call's output buffers (the outputs belong to the call, not to the handle), trace.
                                          The varlen refusal is the model's ValueError and never enters the engine; the group refusal is submit()'s,
                                          ahead of upload_table: both show that a refusal leaves nothing behind, neither reaches vl_tab / vl_host
  test_a_vit_call_refused_behind_its_switches   the same for a vtq_forward_vit call refused by the shared path's checks: its `out` and `states`
  test_after_an_out_of_range_position_under_auto   the error word and _launch_checked behind an IndexError, for rollout, group and varlen
  test_token_num_between_calls            iqa_token set per call by _enqueue; ReferenceFeatures.token
  test_auto_nan_input_*                   _launch_checked's three runs into the same output tensors, the parked fp16x3 engine
  test_auto_nan_reference                 the same through encode_reference: its three runs into `rows`, the precision its ReferenceFeatures records
  test_auto_overflow_*                    _launch_checked's switch to bf16x3 for the calls with several outputs
  test_the_comparator_can_fail            the comparison itself
"""
import ctypes as C
import json
import warnings

import pytest
import torch

from tests import interleave as il
from tests.gpu_util import stream
from vtamiq_amd import VTAMIQ, StaleReferenceError, _lib, synth

pytestmark = pytest.mark.gpu
DEV = il.DEV
MODES = [("fp16x3", 0), ("bf16", 0)]                      # three planes' worth of strides / one plane per activation
MODE_IDS = ["fp16x3", "bf16"]
FULL = ("fp16x3", _lib.OPT_FULL_LAST_LAYER)


def refs_for(names, precision, options=0, **kw):
    return {n: il.reference(n, precision, options, **kw) for n in names}


def run_all(m, names):
    return [(n, il.CATALOGUE[n].run(m)) for n in names]


# pairwise_small first: its last key tile reads the slack rows of `big` behind M_pad = 256, and behind a carrier it is then the call that
# meets them as the carrier left them (forward_small, 168 rows, would clear them on its way without reading them)
SMALL_CALLS = ["pairwise_small"] + [n for n in il.SMALL if n != "pairwise_small"]


def check_small_calls(m, precision, options=0):
    """The small call of every kind on `m`: fresh-engine bits."""
    got = run_all(m, SMALL_CALLS)
    torch.cuda.synchronize()
    lines = il.compare(got, refs_for(il.SMALL, precision, options))
    assert not lines, "\n".join(lines)


# ---- a: any order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,options", MODES + [FULL], ids=MODE_IDS + ["fp16x3_full_last_layer"])
def test_any_order(precision, options):
    """The whole plan (65 calls, every ordered pair of kinds) on one model with no host synchronisation between calls, the returned
    tensors kept as they are: after one synchronize every output of every call -- the first occurrences included, which 60 later calls
    had the chance to overwrite -- has the fresh engine's bits."""
    plan = il.plan()
    refs = refs_for(il.CATALOGUE, precision, options)
    for name, outs in refs.items():
        assert all(bool(torch.isfinite(t).all()) for t in outs), name
    assert il.all_pairs_differ(refs) is None, il.all_pairs_differ(refs)
    m = il.build_model(precision, options)
    for n in set(plan):
        il.CATALOGUE[n].inputs()
    torch.cuda.synchronize()
    got = run_all(m, plan)
    torch.cuda.synchronize()
    m.check_inputs()
    lines = il.compare(got, refs)
    print(f"[any order {precision} options {options}] {len(plan)} calls, {sum(len(o) for _, o in got)} output tensors compared")
    assert not lines, "\n".join(lines[:20])


# ---- b: after a poisoned call ----------------------------------------------------------------------------------------------------------
POISON = [(c, float("nan")) for c in il.CARRIERS] + [("forward_large", float("inf")), ("rollout_large", float("inf"))]


@pytest.mark.parametrize("precision,options", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("carrier,value", POISON, ids=[f"{c}_{'nan' if v != v else 'inf'}" for c, v in POISON])
def test_after_a_poisoned_call(carrier, value, precision, options):
    """One non-finite sample in EVERY image of a large call: every workspace row it touches is non-finite (tests/test_interleave_plan.py:
    at least M_pad + 128 rows of every clean call).  Its scores are all NaN, check_inputs() says so once, and the small call of every
    kind behind it has the fresh engine's bits -- 0 * inf in a masked probability is what the slack-row memsets are there for."""
    e = il.CATALOGUE[carrier]
    m = il.build_model(precision, options)                 # an explicit precision: no re-run
    outs = e.run(m, e.poisoned(value, every_image=True))
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs[0]).all()), outs[0]
    with pytest.raises(FloatingPointError):
        m.check_inputs()
    m.check_inputs()                                        # cleared by the check
    check_small_calls(m, precision, options)
    m.check_inputs()


@pytest.mark.parametrize("precision,options", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("carrier", il.CARRIERS)
def test_one_poisoned_pair(carrier, precision, options):
    """NaN in one image only (the distorted image of pair 1; forward_vit: image 1), on an engine that has run other calls: the NaN mask
    of every output is the fresh engine's, and every output row of a pair without NaN has the bits of the CLEAN call -- scores, rollout
    and last_attention rows, forward_vit's rows, states and maps."""
    e = il.CATALOGUE[carrier]
    inp = e.poisoned(float("nan"), every_image=False)
    want = il.fresh_outputs(carrier, precision, options, inp=inp)
    clean = il.reference(carrier, precision, options)
    m = il.build_model(precision, options)
    run_all(m, ["pairwise_large", "vit_small"])
    outs = e.run(m, inp)
    torch.cuda.synchronize()
    assert len(outs) == len(want) == len(clean) == len(e.pair_axes)
    for k, (a, w, c, axis) in enumerate(zip(outs, want, clean, e.pair_axes)):
        mask = torch.isnan(a)
        assert torch.equal(mask, torch.isnan(w)), (carrier, k)
        bad = mask.movedim(axis, 0).reshape(a.shape[axis], -1).any(1)      # per pair: does this output hold a NaN for it?
        assert bad.tolist() == [i == 1 for i in range(a.shape[axis])], (carrier, k, bad.tolist())
        healthy = [i for i in range(a.shape[axis]) if i != 1]
        for i in healthy:
            assert il.same_bits(a.select(axis, i), c.select(axis, i)), (carrier, k, i)


# ---- c: after a call that fails --------------------------------------------------------------------------------------------------------
def _rollout_buffers():
    """Canary-filled q / rollout / last_attention buffers, large enough for the LARGEST call of the catalogue (6 sequences of S = 302):
    were a switch left set, the call behind the refusal would write a walk of its own size into them -- inside the buffers, where the
    test sees it."""
    return [torch.full(s, 7.0, device=DEV) for s in ((8,), (2, 3, 302), (2, 3, 12, 302))]


def _untouched(*ts):
    return all(bool((t == 7.0).all()) for t in ts)


@pytest.mark.parametrize("precision,options", MODES, ids=MODE_IDS)
def test_after_a_refused_call(precision, options):
    """Calls that include/vtamiq_hip.h says are refused (non-zero, no launch), each between valid calls of other kinds and followed by the
    small call of every kind.  The rollout refusals happen AFTER the entry has taken the call's output pointers: a plain forward behind
    them must leave the refused call's canary-filled output buffers alone."""
    m = il.build_model(precision, options)
    refs = refs_for(["rollout_large", "varlen_large", "group_large", "forward_large"], precision, options)
    lib = m._engine_lib()

    def valid(name):
        got = run_all(m, [name])
        torch.cuda.synchronize()
        lines = il.compare(got, refs)
        assert not lines, "\n".join(lines)

    def ptrs(name):
        inp = il.CATALOGUE[name].inputs()
        return inp, [t.data_ptr() for t in inp["p"]], [t.data_ptr() for t in inp["pos"]]

    # a rollout call with a NULL pos_dist: accepted by vtq_forward_rollout, refused by the shared forward path ("null tensor")
    valid("varlen_large")
    eng = m._engine
    inp, p, ps = ptrs("rollout_small")
    q, roll, last = _rollout_buffers()
    rc = lib.vtq_forward_rollout(eng, p[0], p[1], ps[0], None, None, None, 3, 40, q.data_ptr(), roll.data_ptr(), last.data_ptr(), stream())
    assert rc != 0 and b"null tensor" in lib.vtq_last_error()
    valid("forward_large")                                                  # were the refused call's outputs kept, it would walk a rollout into `roll`
    assert _untouched(q, roll, last)
    check_small_calls(m, precision, options)
    assert _untouched(q, roll, last)

    # a rollout call while a token trace is set
    valid("group_large")
    trace = torch.zeros(3, 6, il.T, 768, device=DEV)
    _lib.check(lib.vtq_set_token_trace(eng, trace.data_ptr()))
    try:
        rc = lib.vtq_forward_rollout(eng, p[0], p[1], ps[0], ps[1], None, None, 3, 40, q.data_ptr(), roll.data_ptr(), last.data_ptr(), stream())
    finally:
        lib.vtq_set_token_trace(eng, None)
    assert rc != 0 and b"token trace" in lib.vtq_last_error()
    valid("forward_large")
    assert _untouched(q, roll, last) and bool((trace == 0).all())
    check_small_calls(m, precision, options)

    # forward_varlen: lengths that do not sum to the tensors' rows (the model refuses it before the engine sees it)
    valid("rollout_large")
    inp = il.CATALOGUE["varlen_small"].inputs()
    with pytest.raises(ValueError):
        m.forward_varlen(inp["p"], inp["pos"], None, il.VL_SMALL[:-1] + [il.VL_SMALL[-1] + 1])
    check_small_calls(m, precision, options)

    # forward_group: a ref_index outside [0, G), through the model and through the C entry
    valid("varlen_large")
    inp, p, ps = ptrs("group_small")
    with pytest.raises(ValueError):
        m.forward_group(inp["p"], inp["pos"], None, [1, 2, 0])
    qg = torch.full((3,), 7.0, device=DEV)
    rc = lib.vtq_forward_group(eng, p[0], p[1], ps[0], ps[1], None, None, 2, 3, 40, (C.c_int32 * 3)(1, 2, 0), qg.data_ptr(), stream())
    assert rc != 0 and b"ref_index" in lib.vtq_last_error()
    valid("rollout_large")
    assert _untouched(qg)
    check_small_calls(m, precision, options)
    m.check_inputs()


SCALES_KW = json.loads(json.dumps(il.KW))
SCALES_KW["vit_config"]["num_scales"] = 2


@pytest.mark.parametrize("precision,options", MODES, ids=MODE_IDS)
def test_a_vit_call_refused_behind_its_switches(precision, options):
    """vtq_forward_vit takes the call's `out` / `states` pointers and is then refused by the shared forward path's checks.  With the catalogue's
    model nothing the shared checks refuse gets past vtq_forward_vit's own, so this case runs on the same model WITH a scale
    embedding: a NULL `scales` is refused there ("required when num_scales > 1").  The pair forward behind it must not copy token rows
    into the refused call's states buffer, and it and a rollout, varlen, group and forward_vit call have the fresh engine's bits."""
    def model():
        m = VTAMIQ(**json.loads(json.dumps(SCALES_KW)), precision=precision, engine_options=options)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, il.WSEED).items()})
        return m.to(DEV).eval()

    m = model()
    pa, po, sc = synth.make_inputs(m.spec, 2, 40, 1201)
    t = lambda a: torch.from_numpy(a).float().to(DEV)
    p, ps, s = (t(pa[:, 0]), t(pa[:, 1])), (t(po[:, 0]), t(po[:, 1])), (t(sc[:, 0]), t(sc[:, 1]))
    flat = lambda ts, *tail: tuple(x.reshape(80, *tail) for x in ts)          # the two pairs as one varlen batch of 30 + 50 patches

    def forward(mm):
        with torch.no_grad():
            return mm(p, ps, s)[0]

    def others(mm):
        with torch.no_grad():
            q, r = mm.forward_rollout(p, ps, s)
            return (q, r.rollout, r.last_attention, mm.forward_varlen(flat(p, 3, 16, 16), flat(ps, 2), flat(s), [30, 50])[0],
                    mm.forward_group(p, ps, s, [1, 0])[0], mm.forward_vit(p[1], ps[1], s[1], tokens_only=True)[0])

    torch.cuda.synchronize()
    fresh = model()
    want = tuple(o.clone() for o in (forward(fresh), *others(fresh)))
    torch.cuda.synchronize()
    del fresh
    assert all(bool(torch.isfinite(o).all()) for o in want)
    with torch.no_grad():
        m.forward_pairwise((p[0], p[1], p[1]), (ps[0], ps[1], ps[1]), (s[0], s[1], s[1]))      # creates the engine; another kind in front
    lib, eng = m._engine_lib(), m._engine
    out = torch.full((2, il.T, 768), 7.0, device=DEV)
    states = torch.full((2, 4, il.T, 768), 7.0, device=DEV)                 # room for the 4 sequences of the calls behind the refusal
    rc = lib.vtq_forward_vit(eng, p[0].data_ptr(), 0, ps[0].data_ptr(), None, 2, 40, 0, out.data_ptr(), states.data_ptr(), None, stream())
    assert rc != 0 and b"scale embedding" in lib.vtq_last_error()
    q = forward(m)                                                          # the pair forward first: it has no such outputs of its own
    torch.cuda.synchronize()
    assert _untouched(out, states)
    got = (q, *others(m))
    torch.cuda.synchronize()
    assert _untouched(out, states)
    assert [il.same_bits(a, b) for a, b in zip(got, want)] == [True] * len(want)
    m.check_inputs()


def test_after_an_out_of_range_position_under_auto():
    """precision="auto": a position of 1.0 raises IndexError from forward_rollout, forward_group and forward_varlen; the error word is
    clear and the small call of every kind behind each has the fresh fp16x3 bits."""
    m = il.build_model("auto")
    for name in ("rollout_small", "group_small", "varlen_small"):
        run_all(m, ["pairwise_large"])
        e = il.CATALOGUE[name]
        inp = {k: tuple(t.clone() for t in v) for k, v in e.inputs().items()}
        inp["pos"][1].view(-1, 2)[3, 1] = 1.0
        with pytest.raises(IndexError):
            e.run(m, inp)
        check_small_calls(m, "fp16x3")
        assert m.engine_precision == "fp16x3"


# ---- d: token_num between calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,options", MODES, ids=MODE_IDS)
def test_token_num_between_calls(precision, options):
    """token_num alternates 0 / 1 from call to call across the kinds (every kind sees both); the reference model is constructed with that
    token.  References encoded at token 0 are refused at token 1 and the call behind the refusal is unaffected."""
    m = il.build_model(precision, options)
    got, want = [], {}
    for i, name in enumerate(il.SMALL + il.SMALL[1:] + il.SMALL[:1]):
        token = i % 2
        m.token_num = token
        got.append((f"{name}@{token}", il.CATALOGUE[name].run(m)))
        want[f"{name}@{token}"] = il.reference(name, precision, options, token=token)
    torch.cuda.synchronize()
    lines = il.compare(got, want)
    assert not lines, "\n".join(lines)
    assert {f"{n}@{t}" for n in il.SMALL for t in (0, 1)} == set(want)
    assert not il.same_bits(want["forward_small@0"][0], want["forward_small@1"][0])       # the token matters
    inp = il.CATALOGUE["cached_small"].inputs()
    m.token_num = 0
    with torch.no_grad():
        ref = m.encode_reference(inp["p"][0], inp["pos"][0], None)
    m.token_num = 1
    with pytest.raises(StaleReferenceError), torch.no_grad():
        m.forward_cached(ref, inp["p"][1], inp["pos"][1], None, il.CACHED_INDEX)
    got = run_all(m, ["rollout_small"])
    torch.cuda.synchronize()
    assert not il.compare(got, {"rollout_small": il.reference("rollout_small", precision, options, token=1)})


# ---- e: the "auto" policy through the entries with several outputs ---------------------------------------------------------------------
# cached_small: encode_reference, then forward_cached.  test_auto_nan_input puts its NaN into the DISTORTED image, so there the re-runs are
# forward_cached's; encode_reference's own are test_auto_nan_reference (NaN) and test_auto_overflow[cached_small] (overflow)
AUTO_ENTRIES = ["rollout_small", "vit_small", "group_small", "pairwise_small", "cached_small"]
NEXT = {"rollout_small": "varlen_small", "vit_small": "rollout_small", "group_small": "vit_small", "pairwise_small": "group_small",
        "cached_small": "pairwise_small"}


@pytest.mark.parametrize("name", AUTO_ENTRIES)
def test_auto_nan_input(name):
    """One NaN input under precision="auto": the launch closure runs fp16x3, bf16x3 and fp16x3 again into the same output tensors.  The
    call returns, with the warning, exactly what an explicit fp16x3 model returns for these inputs -- NaN mask and every other bit of
    EVERY output tensor --, the model stays in fp16x3, and the next clean call of another kind has the fresh fp16x3 bits."""
    e = il.CATALOGUE[name]
    inp = e.poisoned(float("nan"), every_image=False)
    want = il.fresh_outputs(name, "fp16x3", inp=inp)
    assert any(bool(torch.isnan(t).any()) for t in want) and not all(bool(torch.isnan(t).all()) for t in want)
    m = il.build_model("auto")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        outs = e.run(m, inp)
    torch.cuda.synchronize()
    assert any("inf / NaN" in str(x.message) for x in w)
    lines = il.compare_masked(outs, want)
    assert not lines, "\n".join(lines)
    assert m.engine_precision == "fp16x3"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = run_all(m, [NEXT[name]])
    torch.cuda.synchronize()
    assert not any("[VTAMIQ]" in str(x.message) for x in w)
    lines = il.compare(got, refs_for([NEXT[name]], "fp16x3"))
    assert not lines, "\n".join(lines)


def test_auto_nan_reference():
    """encode_reference under precision="auto" with one NaN sample in REFERENCE image 1: its launch closure runs fp16x3, bf16x3 and fp16x3
    again into the same `rows`.  The rows have the NaN mask and elsewhere the bits of an explicit fp16x3 model's, the ReferenceFeatures
    records fp16x3 and the model stays there; forward_cached on them gives that model's scores (NaN exactly where ref_index points at
    reference 1), and the next clean call of another kind has the fresh fp16x3 bits."""
    e = il.CATALOGUE["cached_small"]
    inp = {k: tuple(t.clone() for t in v) for k, v in e.inputs().items()}
    inp["p"][0][1, 7, 1, 3, 3] = float("nan")
    want_rows, want_q = il.fresh_outputs("cached_small", "fp16x3", inp=inp)
    assert torch.isnan(want_rows).any(1).tolist() == [False, True]
    assert torch.isnan(want_q).tolist() == [i == 1 for i in il.CACHED_INDEX]
    m = il.build_model("auto")
    with warnings.catch_warnings(record=True) as w, torch.no_grad():
        warnings.simplefilter("always")
        ref = m.encode_reference(inp["p"][0], inp["pos"][0], None)
    torch.cuda.synchronize()
    assert any("inf / NaN" in str(x.message) for x in w)
    assert ref.precision == "fp16x3" and m.engine_precision == "fp16x3"
    lines = il.compare_masked((ref.rows,), (want_rows,))
    assert not lines, "\n".join(lines)
    with warnings.catch_warnings(record=True), torch.no_grad():
        warnings.simplefilter("always")
        q = m.forward_cached(ref, inp["p"][1], inp["pos"][1], None, il.CACHED_INDEX)[0]
    torch.cuda.synchronize()
    lines = il.compare_masked((ref.rows, q), (want_rows, want_q))          # the rows again: forward_cached only reads them
    assert not lines, "\n".join(lines)
    assert m.engine_precision == "fp16x3"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = run_all(m, ["rollout_small", "cached_small"])
    torch.cuda.synchronize()
    assert not any("[VTAMIQ]" in str(x.message) for x in w)
    lines = il.compare(got, refs_for(["rollout_small", "cached_small"], "fp16x3"))
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("name", AUTO_ENTRIES)
def test_auto_overflow(name):
    """The 1e7-gain attention_norm weights of test_default_model_has_no_silent_nans under precision="auto": the call switches the model
    to bf16x3 with the warning, every output equals an explicit bf16x3 model's, and the following call of another kind runs bf16x3
    directly (no warning, that model's bits)."""
    want = refs_for([name, NEXT[name]], "bf16x3", weights="gain1e7")
    for outs in want.values():
        assert all(bool(torch.isfinite(t).all()) for t in outs)
    m = il.build_model("auto", weights="gain1e7")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = run_all(m, [name])
    assert any("bf16x3" in str(x.message) for x in w)
    assert m.engine_precision == "bf16x3"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got += run_all(m, [NEXT[name]])
    torch.cuda.synchronize()
    assert not any("[VTAMIQ]" in str(x.message) for x in w)
    lines = il.compare(got, want)
    assert not lines, "\n".join(lines)
    assert m.engine_precision == "bf16x3"


# ---- f: the comparator can fail --------------------------------------------------------------------------------------------------------
def test_the_comparator_can_fail():
    """The comparison of test_any_order against references from a model built with token_num = 1 where the model under test uses 0:
    every scoring call is reported, by position and name; against its own references nothing is."""
    names = ["forward_small", "rollout_small", "group_small"]
    m = il.build_model("fp16x3")
    got = run_all(m, names)
    torch.cuda.synchronize()
    assert il.compare(got, refs_for(names, "fp16x3")) == []
    lines = il.compare(got, refs_for(names, "fp16x3", token=1))
    for i, n in enumerate(names):
        assert any(line.startswith(f"call {i} {n} output 0:") for line in lines), lines
    assert il.compare(got[:1], {"forward_small": got[0][1] + got[0][1]}) == ["call 0 forward_small: 1 outputs, the fresh engine gives 2"]
