"""The stream and concurrency contract of the library (include/vtamiq_hip.h: asynchronous on the stream passed in; DESIGN.md section 1,
"Streams and concurrency"): engines on side streams, several engines at once on several streams and from several threads, one engine moved
between streams by the caller's events, the loader pipeline under a non-default current stream -- and the process-wide GEMM schedule
cache used from a stream that did not upload the schedule.

Every case compares with the SAME computation done serially on the default stream after a full synchronize, bit for bit (torch.equal:
bit-identity is the project's own claim, test_gpu_parity.test_repeated_forwards_are_bitwise_identical), so no tolerance is introduced
here; where a reference-scored fixture or an fp64 bound exists for the computation (the goldens' gate, test_gemm_bias's bound), that
is asserted as well.  A stream is kept busy with a bounded chain of torch matmuls into a scratch tensor (a few tens of ms), never
with a spin.  At most 4 streams: a process has 4 hardware queues.

The cases that need process state nobody has touched (an unseen schedule key; every kernel's first-use configuration raced by
threads) run in a child process: `python -m tests.test_gpu_streams <case> ...` (main() below)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import interleave as il
from tests.gpu_util import FORMATS, elt_dtype, num_code, planes_value, to_planes
from tests.helpers import gate_error, load_case, split_inputs
from vtamiq_amd import VTAMIQ, _lib, synth
from vtamiq_amd.spec import make_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL = {"fp16x3": 1e-3, "fp16": 3e-2}                    # the goldens' gate, as in test_gpu_parity.TOL
VITB = dict(vit_config=dict(variant="ViT-B16", pretrained=False))
VITL = dict(vit_config=dict(variant="ViT-L16", pretrained=False))
SMALL = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False))


class Busy:
    """Bounded unrelated work for a stream: `n` fp32 matmuls of 6144^3 into a scratch tensor (about 5 ms each on an MI355X).  The first
    product runs at construction on the current stream, so that the BLAS library's own first-use work is not part of a test."""

    def __init__(self):
        g = torch.Generator(device="cpu").manual_seed(1)
        self.a = torch.randn(6144, 6144, generator=g).to(DEV)
        self.b = self.a.t().contiguous()
        self.out = torch.empty_like(self.a)
        torch.mm(self.a, self.b, out=self.out)
        torch.cuda.synchronize()

    def __call__(self, stream, n=6):
        with torch.cuda.stream(stream):
            for _ in range(n):
                torch.mm(self.a, self.b, out=self.out)


@pytest.fixture(scope="module")
def busy():
    return Busy()


def make_model(kw, sd_np, precision, layers=False, attention=False):
    """A model on the device with `sd_np` loaded; the parameter copies go onto the CURRENT stream, the engine is not created yet."""
    m = VTAMIQ(**json.loads(json.dumps(kw)), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    m.transformer.encoder.return_layers = layers
    m.transformer.encoder.return_attention = attention
    return m.to(DEV).eval()


def seeded(kw, precision, wseed, B, N, iseed):
    """-> (model, forward() arguments) from the seeded generators; inputs on the device, made on the current stream."""
    spec = make_spec(**json.loads(json.dumps(kw)))
    m = make_model(kw, synth.make_state_dict(spec, wseed), precision)
    return m, split_inputs(*synth.make_inputs(spec, B, N, iseed), device=DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- cold start on a side stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("name", ["c1_b2_n50", "c2_b32_n500"])
def test_cold_start_on_a_side_stream(name, precision, busy):
    """A model's very first forward -- parameter upload, engine creation, weight packing, workspace reserve, schedule upload, the
    launches -- inside torch.cuda.stream(side) while the default stream is busy: the scores of a second model with the same weights run
    on the default stream, and the reference's scores for the fixture within the goldens' gate.  B = 2, N = 50: the small-tile GEMMs and
    the 4-wave attention kernel; B = 32, N = 500: the persistent GEMM and (fp16x3) the pipelined attention kernel."""
    g, kw, spec, sd, (patches, pos, scales) = load_case(name)
    args = split_inputs(patches, pos, scales, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    busy(torch.cuda.default_stream())
    with torch.cuda.stream(side), torch.no_grad():
        q_side = make_model(kw, sd, precision)(*args)[0]
    torch.cuda.synchronize()
    with torch.no_grad():
        q_main = make_model(kw, sd, precision)(*args)[0]
    torch.cuda.synchronize()
    assert same_bits(q_side, q_main), (q_side - q_main).abs().max().item()
    q = q_side.cpu().numpy()
    if precision == "fp16x3":
        assert gate_error(q, g["q"]) < TOL[precision], gate_error(q, g["q"])
    else:       # single plane: gated on the batch's rms at the bench size (test_golden_at_the_bench_sizes says why), raw on the small fixture
        rms = float(np.sqrt(np.mean(g["q"].astype(np.float64) ** 2)))
        err = float(np.abs(q - g["q"]).max() / rms) if name == "c2_b32_n500" else gate_error(q, g["q"])
        assert err < TOL[precision], err


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_cold_start_on_a_side_stream_pairwise_and_vit(precision, busy):
    """The same for the two other entry points at the small shape: forward_pairwise, and forward_vit with every token row, the layer
    states and the attention maps -- each the first call of a fresh model, on a side stream under a busy default stream."""
    g, kw, spec, sd, (patches, pos, scales) = load_case("c1_b2_n50")
    (p0, p1), (s0, s1), sc = split_inputs(patches, pos, scales, device=DEV)
    p2 = p1.flip(0).contiguous()
    trip = ((p0, p1, p2), (s0, s1, s1), (sc[0], sc[1], sc[1]))
    side = torch.cuda.Stream()

    def pairwise():
        return list(make_model(kw, sd, precision).forward_pairwise(*trip))

    def vit():
        x, probs, states = make_model(kw, sd, precision, layers=True, attention=True).forward_vit(p1, s1, sc[1], tokens_only=False)
        assert len(probs) == spec.num_layers and len(states) == spec.num_layers
        return [x] + probs + states

    got = {}
    for call in (pairwise, vit):
        torch.cuda.synchronize()
        busy(torch.cuda.default_stream())
        with torch.cuda.stream(side), torch.no_grad():
            got[call] = call()
        torch.cuda.synchronize()
        with torch.no_grad():
            want = call()
        torch.cuda.synchronize()
        assert len(got[call]) == len(want)
        for i, (a, b) in enumerate(zip(got[call], want)):
            assert same_bits(a, b), (call.__name__, i)
    # (ref, dist1) is the fixture's pair: the first pairwise score against the reference's, within the goldens' gate
    err = gate_error(got[pairwise][0].cpu().numpy(), g["q"])
    assert err < TOL[precision], err
    assert not torch.equal(got[pairwise][0], got[pairwise][1])


# ---- the schedule cache from a stream that did not upload ---------------------------------------------------------------------------
def child(*argv, timeout=600):
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_streams", *argv], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])


@pytest.mark.parametrize("fmt", ["fp16x3", "fp16"])
def test_cached_schedule_is_usable_from_a_stream_that_did_not_upload_it(fmt):
    """child_schedule below, in a fresh process (the cache is process-wide and the shape must be unseen)."""
    child("schedule", fmt)


def child_schedule(fmt):
    """The persistent kernel forced, a tile grid (7 x 5) nothing else in the process has used.  Stream A is busy; vtq_k_gemm for the
    shape goes onto A (first use: the schedule is built and uploaded) and at once onto B with other operands and a poisoned output
    (the cache answers).  B's output -- and A's -- equal the same call repeated on the default stream after a synchronize, bit for
    bit, and meet test_gemm_bias's fp64 bound for the format."""
    from tests.test_gpu_kernels import OUT_TOL
    lib = _lib.load()
    M, N, K = 1792, 1280, 512                       # K: a multiple of two K tiles in both formats (128 for one plane, 64 for three terms)
    busy = Busy()

    def randn(*s, seed, scale=1.0):
        return (torch.randn(*s, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale).to(DEV)

    def poisoned(planes):
        return torch.full((planes, M, N), float("nan"), dtype=elt_dtype(fmt), device=DEV)

    ops = []
    for seed in (100, 200):
        A, W, bias = randn(M, K, seed=seed), randn(N, K, seed=seed + 1, scale=0.05), randn(N, seed=seed + 2)
        ops.append((A, W, bias, to_planes(A, fmt, "a"), to_planes(W, fmt, "w")))
    outs = [poisoned(o[3].shape[0]) for o in ops]
    again = [poisoned(o[3].shape[0]) for o in ops]

    def gemm(o, out, stream):
        _, _, bias, Ap, Wp = o
        _lib.check(lib.vtq_k_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, num_code(fmt), 0, bias.data_ptr(), None, None,
                                  out.data_ptr(), M * N, N, stream.cuda_stream))

    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    _lib.check(lib.vtq_debug_gemm_variant(0))
    try:
        torch.cuda.synchronize()
        busy(sa)
        gemm(ops[0], outs[0], sa)
        gemm(ops[1], outs[1], sb)
        torch.cuda.synchronize()
        for o, out in zip(ops, again):
            gemm(o, out, torch.cuda.default_stream())
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.vtq_debug_gemm_variant(-1))
    tol = OUT_TOL[fmt]
    for which, (o, out, rep) in enumerate(zip(ops, outs, again)):
        A, W, bias, Ap, Wp = o
        assert same_bits(out, rep), which
        ref = planes_value(Ap) @ planes_value(Wp).t() + bias.double()
        got = planes_value(out)
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"[schedule {fmt}] stream {'AB'[which]}: err {err:.3e} (bound {tol:g})")
        assert err < tol, err
        assert torch.allclose(got, ref, rtol=0, atol=tol * ref.abs().max().item())
        if FORMATS[fmt][1] == 3:
            exact = A.double() @ W.double().t() + bias.double()
            assert (got - exact).abs().max().item() < 2e-5 * exact.abs().max().item()


# ---- K engines on K streams ---------------------------------------------------------------------------------------------------------
SERVING = [(VITB, "fp16x3", 1, 500)] * 4
# kernels that overlap: B = 32 fp16x3 runs the 160 KiB-LDS persistent GEMM and the pipelined attention kernel, B = 1 the small tiles
MIXED = [(VITB, "fp16x3", 32, 500), (VITB, "fp16x3", 1, 500), (VITB, "bf16", 4, 500), (VITL, "bf16x3", 2, 200)]


def engine_set(configs):
    """One model per entry, each with its own weight seed and its own inputs."""
    return [seeded(kw, precision, 40 + i, B, N, 140 + i) for i, (kw, precision, B, N) in enumerate(configs)]


def serial_scores(models):
    """Every model's scores on the default stream, one after the other -- and they differ from model to model, so that equality with
    them is no empty statement and an engine that computed with another engine's workspace, weights or schedule would be seen."""
    torch.cuda.synchronize()
    want = []
    with torch.no_grad():
        for m, args in models:
            want.append(m(*args)[0].clone())
            torch.cuda.synchronize()
    firsts = [w[0].item() for w in want]
    assert all(np.isfinite(firsts)) and len(set(firsts)) == len(firsts), firsts
    return want


@pytest.mark.parametrize("configs,rounds", [(SERVING, 6), (MIXED, 4)], ids=["serving_4x_b1", "mixed_kernels"])
def test_engines_on_their_own_streams_round_robin(configs, rounds):
    """The pattern of tools/concurrent_streams.py: K = 4 engines on 4 streams, `rounds` rounds enqueued round-robin with no host
    synchronisation in between, the first round each engine's cold start.  Every round of every engine gives that model's serial
    scores."""
    models = engine_set(configs)
    streams = [torch.cuda.Stream() for _ in models]
    torch.cuda.synchronize()
    got = [[] for _ in models]
    with torch.no_grad():
        for _ in range(rounds):
            for i, (m, args) in enumerate(models):
                with torch.cuda.stream(streams[i]):
                    got[i].append(m(*args)[0])
    torch.cuda.synchronize()
    want = serial_scores(models)
    for i, qs in enumerate(got):
        for r, q in enumerate(qs):
            assert same_bits(q, want[i]), (i, r)


def test_engines_on_their_own_threads():
    """child_threads below, in a fresh process: the first-use paths of the whole library are untouched when the threads start."""
    child("threads", timeout=900)


def child_threads(rounds=3):
    """The mixed set from 4 Python threads, one model and one stream each, released together by a barrier.  ctypes drops the GIL around
    every library call, so the mutex-guarded first-use paths -- the schedule cache, every kernel's configured[] table, the attention
    CU-count cache -- are entered concurrently on the host.  Each thread's scores, every round, are its model's serial scores."""
    models = engine_set(MIXED)
    streams = [torch.cuda.Stream() for _ in models]
    torch.cuda.synchronize()
    got, errors = [[] for _ in models], []
    start = threading.Barrier(len(models))

    def work(i):
        try:
            m, args = models[i]
            start.wait(timeout=60)
            with torch.cuda.stream(streams[i]), torch.no_grad():
                for _ in range(rounds):
                    got[i].append(m(*args)[0])
            streams[i].synchronize()
        except BaseException as e:                                        # reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(models))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors and not any(t.is_alive() for t in threads), errors
    torch.cuda.synchronize()
    want = serial_scores(models)
    for i, qs in enumerate(got):
        assert len(qs) == rounds
        for r, q in enumerate(qs):
            assert same_bits(q, want[i]), (i, r)


# ---- the entries added since: rollout, varlen, group / cached, forward_vit with maps -------------------------------------------------
# four models, each with its own weight seed, each running a short fixed list of calls of tests/interleave.py's catalogue: the rollout
# workspace regrows (small, then large), varlen's tables and the group / cached ref_index go through each engine's own vl_tab and pinned
# image, forward_vit's per-call switches sit in front of a plain forward
ENTRIES = [["rollout_small", "rollout_large"], ["varlen_small", "varlen_large"], ["group_small", "cached_small"], ["vit_large", "forward_small"]]


def entry_models():
    """One fp16x3 model per list of ENTRIES (weight seeds 90 ..); every input of the lists on the device before anything runs."""
    for names in ENTRIES:
        for n in names:
            il.CATALOGUE[n].inputs()
    return [il.build_model("fp16x3", wseed=90 + i) for i in range(len(ENTRIES))]


def serial_entries(models):
    """Every model's list on the default stream, one call after the other, cloned -- finite, and different from model to model."""
    torch.cuda.synchronize()
    want = []
    for m, names in zip(models, ENTRIES):
        outs = []
        for n in names:
            outs.append(tuple(t.clone() for t in il.CATALOGUE[n].run(m)))
            torch.cuda.synchronize()
        want.append(outs)
    assert all(bool(torch.isfinite(t).all()) for outs in want for o in outs for t in o)
    firsts = [outs[-1][0].flatten()[0].item() for outs in want]
    assert len(set(firsts)) == len(firsts), firsts
    return want


def same_entries(got, want, who):
    """got: one run of a model's list (a tuple of tensors per call) against the serial run's."""
    assert len(got) == len(want), who
    for c, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (who, c)
        for k, (x, y) in enumerate(zip(a, b)):
            assert il.same_bits(x, y), (who, c, k)


def test_new_entries_on_their_own_streams_round_robin():
    """ENTRIES on 4 streams, 3 rounds enqueued round-robin with no host synchronisation in between, the first round each engine's cold
    start: every output of every call of every round has the bits of the serial default-stream run."""
    models = entry_models()
    streams = [torch.cuda.Stream() for _ in models]
    torch.cuda.synchronize()
    rounds = 3
    got = [[] for _ in models]
    for _ in range(rounds):
        for i, (m, names) in enumerate(zip(models, ENTRIES)):
            with torch.cuda.stream(streams[i]):
                got[i].append([il.CATALOGUE[n].run(m) for n in names])
    torch.cuda.synchronize()
    want = serial_entries(models)
    for i, runs in enumerate(got):
        for r, run in enumerate(runs):
            same_entries(run, want[i], (i, r))


def test_new_entries_on_their_own_threads():
    """child_entries below, in a fresh process."""
    child("entries", timeout=900)


def child_entries(rounds=3):
    """ENTRIES from 4 Python threads, one model and one stream each, released together by a barrier, as child_threads: each thread's
    outputs, every round, are its model's serial outputs."""
    models = entry_models()
    streams = [torch.cuda.Stream() for _ in models]
    torch.cuda.synchronize()
    got, errors = [[] for _ in models], []
    start = threading.Barrier(len(models))

    def work(i):
        try:
            start.wait(timeout=60)
            with torch.cuda.stream(streams[i]):
                for _ in range(rounds):
                    got[i].append([il.CATALOGUE[n].run(models[i]) for n in ENTRIES[i]])
            streams[i].synchronize()
        except BaseException as e:                                        # reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(models))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors and not any(t.is_alive() for t in threads), errors
    torch.cuda.synchronize()
    want = serial_entries(models)
    for i, runs in enumerate(got):
        assert len(runs) == rounds
        for r, run in enumerate(runs):
            same_entries(run, want[i], (i, r))


# ---- one engine, several streams, ordered by the caller ---------------------------------------------------------------------------------
def test_one_engine_alternating_streams_ordered_by_events(busy):
    """One handle is used by one stream at a time, and the caller's events say which: forward on A; B waits for A's event and runs a
    LARGER batch (the workspace regrows); A waits for B's and runs the first inputs again.  All three equal a second model's scores on
    the default stream."""
    spec = make_spec(**json.loads(json.dumps(SMALL)))
    sd = synth.make_state_dict(spec, 61)
    x1 = split_inputs(*synth.make_inputs(spec, 2, 50, 62), device=DEV)
    x2 = split_inputs(*synth.make_inputs(spec, 9, 300, 63), device=DEV)
    ref, m = make_model(SMALL, sd, "fp16x3"), make_model(SMALL, sd, "fp16x3")
    with torch.no_grad():
        want = [ref(*x1)[0].clone(), ref(*x2)[0].clone()]
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    busy(A, n=3)
    with torch.no_grad():
        with torch.cuda.stream(A):
            q1 = m(*x1)[0]
        B.wait_event(A.record_event())
        with torch.cuda.stream(B):
            q2 = m(*x2)[0]
        A.wait_event(B.record_event())
        with torch.cuda.stream(A):
            q3 = m(*x1)[0]
    torch.cuda.synchronize()
    assert same_bits(q1, want[0]) and same_bits(q2, want[1]) and same_bits(q3, want[0])
    assert not torch.equal(want[0], want[1][:2])


def test_input_error_word_is_read_and_cleared_in_stream_order(busy):
    """precision="auto" reads the engine's error word after every forward, on the forward's stream.  One out-of-range position in a side
    stream raises the IndexError the default stream raises, and the next clean forward there passes with the default stream's bits:
    the word was read behind the forward that set it and cleared ahead of the next."""
    spec = make_spec(**json.loads(json.dumps(SMALL)))
    sd = synth.make_state_dict(spec, 71)
    p, ps, sc = split_inputs(*synth.make_inputs(spec, 2, 50, 72), device=DEV)
    bad = ps[0].clone()
    bad[1, 3, 0] = 1.5
    ref, m = make_model(SMALL, sd, "auto"), make_model(SMALL, sd, "auto")
    with torch.no_grad():
        with pytest.raises(IndexError) as main_err:
            ref(p, (bad, ps[1]), sc)
        want = ref(p, ps, sc)[0].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy(torch.cuda.default_stream(), n=3)
    with torch.cuda.stream(side), torch.no_grad():
        with pytest.raises(IndexError) as side_err:
            m(p, (bad, ps[1]), sc)
        q = m(p, ps, sc)[0]
        q_again = m(p, ps, sc)[0]
    torch.cuda.synchronize()
    assert str(side_err.value) == str(main_err.value)
    assert same_bits(q, want) and same_bits(q_again, want)
    assert m.engine_precision == "fp16x3" and ref.engine_precision == "fp16x3"


# ---- the loader pipeline under a non-default current stream ---------------------------------------------------------------------------
def test_image_pair_pipeline_under_a_side_stream(busy):
    """The body of test_gpu_parity.test_image_pair_pipeline_matches_the_direct_path (one scale) with a side stream current: the pipeline
    is built there, copies on its own stream and gathers and forwards on the side stream, five batches over two buffer sets, while the
    default stream is busy.  The scores equal extract_patches + the model called directly on the default stream afterwards."""
    from vtamiq_amd.patches import extract_patches
    from vtamiq_amd.pipeline import ImagePairPipeline
    spec = make_spec(**json.loads(json.dumps(SMALL)))
    m = make_model(SMALL, synth.make_state_dict(spec, 3), "fp16x3")
    B, N, H, W = 3, 60, 96, 128
    rs = np.random.RandomState(5)
    batches = []
    for _ in range(5):
        ref = rs.randint(0, 256, size=(B, H, W, 3), dtype=np.uint8)
        dist = rs.randint(0, 256, size=(B, H, W, 3), dtype=np.uint8)
        smp = np.stack([rs.randint(0, H - 15, size=(B, N)), rs.randint(0, W - 15, size=(B, N))], axis=-1).astype(np.int32)
        batches.append((ref, dist, smp))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    busy(torch.cuda.default_stream())
    with torch.cuda.stream(side):
        pipe = ImagePairPipeline(m, B, (H, W), N)
        got = [pipe.submit(ref, dist, smp) for ref, dist, smp in batches]
    torch.cuda.synchronize()
    for (ref, dist, smp), q in zip(batches, got):
        img = torch.from_numpy(np.concatenate([ref, dist])).to(DEV)
        s2 = torch.from_numpy(np.concatenate([smp, smp])).to(DEV)
        pa, po, sc = extract_patches(img, s2, None, 1)
        with torch.no_grad():
            want = m((pa[:B], pa[B:]), (po[:B], po[B:]), (sc[:B], sc[B:]) if sc is not None else (None, None))[0]
        torch.cuda.synchronize()
        assert same_bits(q, want)
    assert not torch.equal(got[0], got[1])


def main(argv):
    case, rest = argv[0], argv[1:]
    {"schedule": child_schedule, "threads": child_threads, "entries": child_entries}[case](*rest)
    print("child ok")


if __name__ == "__main__":
    main(sys.argv[1:])
