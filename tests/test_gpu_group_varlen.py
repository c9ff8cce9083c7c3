"""forward_group / encode_reference / forward_cached with `lengths=` on the GPU: one-to-many scoring on images of different patch counts.

The contract every test here turns on: a sequence never depends on what else is in the batch.  Row g of encode_reference(lengths) has the BITS
of encode_reference on reference g alone, q[m] of forward_cached(lengths) the bits of forward_cached on image m alone, forward_group(lengths)
the bits of that chain -- and, where a distorted image has its reference's patch count, of the model on the single pair.  The oracle comparison
beside the bit checks keeps them from being vacuous (two equal wrong answers)."""
import ctypes as C
import functools
import json
import warnings

import numpy as np
import pytest
import torch

from oracle import vtamiq_oracle as O
from tests.gpu_util import stream
from tests.helpers import rel_err
from tests.test_gpu_footprint import Layout
from tests.test_gpu_group import _group
from tests.test_gpu_parity import TOL, gate
from tests.test_gpu_varlen import CONFIGS as VARLEN_CONFIGS
from tests.test_gpu_varlen import _model
from vtamiq_amd import VTAMIQ, _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
bits32 = lambda t: t.contiguous().view(torch.int32)

# ViT-B/16 without register tokens: S = 9, 64, 65, 128, 201 -- either side of the 64-key tile and the 128-row query block
N_REF = [8, 63, 64, 127, 200]
N_DIST = [8, 64, 63, 130, 127, 200, 77, 56, 1, 200]
INDEX = [0, 1, 1, 3, 3, 4, 2, 0, 2, 4]         # equal counts: images 0, 2, 4, 5, 9 (reference 4 twice); every reference is used
PRECISIONS = ["fp16x3", "bf16x3", "fp16", "auto"]


def _case(name, T):
    """(n_ref, n_dist, ref_index) of a configuration: the case above -- ViT-L/16 on three lengths -- plus, when the CLS fold's chunk is at most
    256 rows, a reference and a distorted image at S = chunk and at S = chunk + 1 (a sequence of exactly one chunk, and one row into the next)."""
    if name == "vit_l16":
        return [8, 130, 63], [130, 8, 63, 8], [1, 0, 2, 1]
    n_ref, n_dist, index = list(N_REF), list(N_DIST), list(INDEX)
    chunk = _lib.load().vtq_k_cls_fold_chunk_rows()
    if chunk <= 256 and chunk - T >= 1:
        g = len(n_ref)
        n_ref += [chunk - T, chunk + 1 - T]
        n_dist += [chunk + 1 - T, chunk - T]
        index += [g + 1, g]                     # equal counts, crosswise
    return n_ref, n_dist, index


def _images(spec, counts, seed, like=None):
    """Per-image CPU tensors [(patches (n, 3, P, P), pos (n, 2), scales (n,) | None)].  like = (references, ref_index): a distorted image with
    its reference's count is that reference plus noise at positions of its own; any other count gives an image of its own."""
    out = []
    for i, n in enumerate(counts):
        pa, po, sc = synth.make_inputs(spec, 1, n, seed + i, aligned=False)
        p = torch.from_numpy(pa[0, 1 if like else 0]).float()
        if like and like[0][like[1][i]][0].shape[0] == n:
            r = np.random.RandomState(seed + 1000 + i)
            p = (like[0][like[1][i]][0] + torch.from_numpy(0.1 * r.normal(size=tuple(p.shape))).float()).clamp(-1.0, 1.0)
        out.append((p, torch.from_numpy(po[0, 1 if like else 0]).float(), None if sc is None else torch.from_numpy(sc[0, 1 if like else 0]).float()))
    return out


def _cat(imgs, device=DEV):
    """The concatenated (patches, pos, scales) a `lengths=` call takes for one image."""
    return tuple(None if imgs[0][k] is None else torch.cat([im[k] for im in imgs]).to(device) for k in range(3))


def _one(im, device=DEV):
    """One image as the uniform entries take it: a batch of 1."""
    return tuple(None if t is None else t[None].to(device) for t in im)


def _data(spec, name, seed=300):
    n_ref, n_dist, index = _case(name, spec.num_tokens)
    refs = _images(spec, n_ref, seed)
    return n_ref, n_dist, index, refs, _images(spec, n_dist, seed + 100, like=(refs, index))


@functools.lru_cache(maxsize=None)
def _oracle_scores(name):
    """The reference forward (oracle, on the host): vit_tokens per image, then the head on (reference ref_index[m], distorted m).  Once per
    configuration, shared by the precisions."""
    vit, _, _ = VARLEN_CONFIGS[name]
    from tests.test_gpu_varlen import _kw
    m = VTAMIQ(**json.loads(json.dumps(_kw(vit))), precision="bf16")
    sd = O.to_torch(synth.make_state_dict(m.spec, 71))
    _, _, index, refs, dists = _data(m.spec, name)
    tok = lambda im: O.vit_tokens(sd, m.spec, im[0][None], im[1][None], None if im[2] is None else im[2][None])
    t_ref, t_dist = [tok(im) for im in refs], [tok(im) for im in dists]
    return np.array([float(O.head(sd, m.spec, t_ref[i], t_dist[k])[0]) for k, i in enumerate(index)])


# ---- 1: bits, end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(VARLEN_CONFIGS))
def test_every_sequence_has_the_bits_of_the_image_alone(name, precision):
    vit, options, _ = VARLEN_CONFIGS[name]
    m, _ = _model(vit, precision, options)
    n_ref, n_dist, index, refs, dists = _data(m.spec, name)
    G, M = len(n_ref), len(n_dist)
    R, D = _cat(refs), _cat(dists)
    with torch.no_grad():
        ref = m.encode_reference(*R, lengths=n_ref)
        for g in range(G):                                                     # rows: each reference alone
            alone = m.encode_reference(*_one(refs[g]))
            assert torch.equal(bits32(ref.rows[g]), bits32(alone.rows[0])), ("rows", g, n_ref[g])
        qc = m.forward_cached(ref, *D, index, lengths=torch.tensor(n_dist))[0]
        q1 = torch.cat([m.forward_cached(ref, *_one(dists[k]), [index[k]])[0] for k in range(M)])      # each distorted image alone
        qg, aux = m.forward_group((R[0], D[0]), (R[1], D[1]), (R[2], D[2]), index, lengths=(n_ref, n_dist))
        equal = [k for k in range(M) if n_dist[k] == n_ref[index[k]]]
        pair = lambda a, b: (None, None) if a is None else (a, b)
        qp = torch.cat([m(*[pair(a, b) for a, b in zip(_one(refs[index[k]]), _one(dists[k]))])[0] for k in equal])     # the pair alone
        perm = list(np.random.RandomState(5).permutation(M))
        Dp = _cat([dists[k] for k in perm])
        qperm = m.forward_group((R[0], Dp[0]), (R[1], Dp[1]), (R[2], Dp[2]), [index[k] for k in perm], lengths=(n_ref, [n_dist[k] for k in perm]))[0]
        as_list = lambda imgs, k: None if imgs[0][k] is None else [im[k].to(DEV) for im in imgs]      # lists of per-image tensors
        ql = m.forward_group((as_list(refs, 0), as_list(dists, 0)), (as_list(refs, 1), as_list(dists, 1)), (as_list(refs, 2), as_list(dists, 2)),
                             index, lengths=(torch.tensor(n_ref), n_dist))[0]
    assert aux is None and qg.shape == (M,) and qg.dtype == torch.float32 and bool(torch.isfinite(qg).all())
    assert len(equal) >= 3 and len(equal) < M
    assert torch.equal(bits32(qc), bits32(q1)), ("cached", (qc - q1).abs().max().item())
    assert torch.equal(bits32(qg), bits32(qc)), ("group", (qg - qc).abs().max().item())
    assert torch.equal(bits32(qg[equal]), bits32(qp)), ("pair", (qg[equal] - qp).abs().max().item())
    assert torch.equal(bits32(qperm), bits32(qg[perm]))
    assert torch.equal(bits32(ql), bits32(qg))
    m.check_inputs()
    want = _oracle_scores(name)
    e = rel_err(qg.cpu().numpy(), want)
    print(f"\n[group varlen {name} {precision}] {e}")
    assert gate(qg.cpu().numpy(), want, TOL["fp16x3" if precision == "auto" else precision]), e


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["plain", "tokens8_layerscale", "full_last_layer", "adapters"])
def test_equal_lengths_are_the_uniform_entries(name, precision):
    vit, options, _ = VARLEN_CONFIGS[name]
    m, _ = _model(vit, precision, options)
    G, M, N, index = 3, 7, 50, [2, 0, 0, 1, 2, 2, 0]
    (pr, pd), (qr, qd), sc = (tuple(None if t is None else t.to(DEV) for t in x) for x in _group(m.spec, G, M, N, index))
    flat = lambda t: None if t is None else t.flatten(0, 1)
    with torch.no_grad():
        q = m.forward_group((pr, pd), (qr, qd), sc, index)[0]
        v = m.forward_group((flat(pr), flat(pd)), (flat(qr), flat(qd)), (flat(sc[0]), flat(sc[1])), index, lengths=([N] * G, [N] * M))[0]
        ref = m.encode_reference(pr, qr, sc[0])
        ref_v = m.encode_reference(flat(pr), flat(qr), flat(sc[0]), lengths=[N] * G)
        c = m.forward_cached(ref, pd, qd, sc[1], index)[0]
        c_v = m.forward_cached(ref_v, flat(pd), flat(qd), flat(sc[1]), index, lengths=[N] * M)[0]
    assert torch.equal(bits32(v), bits32(q))
    assert torch.equal(bits32(ref_v.rows), bits32(ref.rows))
    assert torch.equal(bits32(c_v), bits32(c)) and torch.equal(bits32(c), bits32(q))


# ---- 2: isolation and the input policy -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    return _model(dict(variant="ViT-B16"), "fp16x3")[0]


def _group_args(R, D):
    return (R[0], D[0]), (R[1], D[1]), (R[2], D[2])


def test_nan_images_reach_only_their_own_scores(plain):
    m = plain
    n_ref, n_dist, index, refs, dists = _data(m.spec, "plain", seed=600)
    R, D = _cat(refs), _cat(dists)
    d0, r0 = np.concatenate([[0], np.cumsum(n_dist)]), np.concatenate([[0], np.cumsum(n_ref)])
    M = len(n_dist)
    with torch.no_grad():
        q = m.forward_group(*_group_args(R, D), index, lengths=(n_ref, n_dist))[0]
        m.check_inputs()
        k = 3                                                                   # one distorted image all NaN
        bad = D[0].clone()
        bad[d0[k]:d0[k + 1]] = float("nan")
        qd = m.forward_group(*_group_args(R, (bad, D[1], D[2])), index, lengths=(n_ref, n_dist))[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        ref = m.encode_reference(*R, lengths=n_ref)
        qcd = m.forward_cached(ref, bad, D[1], D[2], index, lengths=n_dist)[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        g = 1                                                                   # one reference all NaN
        bad = R[0].clone()
        bad[r0[g]:r0[g + 1]] = float("nan")
        qr = m.forward_group(*_group_args((bad, R[1], R[2]), D), index, lengths=(n_ref, n_dist))[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        ref_bad = m.encode_reference(bad, R[1], R[2], lengths=n_ref)
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        qcr = m.forward_cached(ref_bad, *D, index, lengths=n_dist)[0]
        with pytest.raises(FloatingPointError):                                 # the NaN rows reach the difference: reported, and the flags cleared
            m.check_inputs()
    keep = [i for i in range(M) if i != k]
    for got in (qd, qcd):
        assert bool(torch.isnan(got[k])) and torch.equal(bits32(got[keep]), bits32(q[keep]))
    hit = [i for i in range(M) if index[i] == g]
    keep = [i for i in range(M) if index[i] != g]
    assert len(hit) == 2
    for got in (qr, qcr):
        assert bool(torch.isnan(got[hit]).all()) and torch.equal(bits32(got[keep]), bits32(q[keep]))
    rows_keep = [i for i in range(len(n_ref)) if i != g]
    assert bool(torch.isnan(ref_bad.rows[g]).all()) and torch.equal(bits32(ref_bad.rows[rows_keep]), bits32(ref.rows[rows_keep]))


def test_check_inputs_reports_a_position_out_of_range_in_any_one_image(plain):
    m = plain
    n_ref, n_dist, index, refs, dists = _data(m.spec, "plain", seed=650)
    R, D = _cat(refs), _cat(dists)
    r0, d0 = np.concatenate([[0], np.cumsum(n_ref)]), np.concatenate([[0], np.cumsum(n_dist)])
    with torch.no_grad():
        ref = m.encode_reference(*R, lengths=n_ref)
        m.check_inputs()
        for g in range(len(n_ref)):                                             # the last patch of each reference in turn
            bad = R[1].clone()
            bad[r0[g + 1] - 1, g & 1] = 1.5 if g & 2 else -0.25
            m.forward_group(*_group_args((R[0], bad, R[2]), D), index, lengths=(n_ref, n_dist))
            with pytest.raises(IndexError):
                m.check_inputs()
            m.encode_reference(R[0], bad, R[2], lengths=n_ref)
            with pytest.raises(IndexError):
                m.check_inputs()
        for k in range(len(n_dist)):                                            # the first patch of each distorted image in turn
            bad = D[1].clone()
            bad[d0[k], k & 1] = float("nan") if k % 3 == 0 else 1.0
            m.forward_group(*_group_args(R, (D[0], bad, D[2])), index, lengths=(n_ref, n_dist))
            with pytest.raises(IndexError):
                m.check_inputs()
            m.forward_cached(ref, D[0], bad, D[2], index, lengths=n_dist)
            with pytest.raises(IndexError):
                m.check_inputs()
        m.forward_group(*_group_args(R, D), index, lengths=(n_ref, n_dist))
        m.check_inputs()                                                        # the flags were cleared: a clean call is clean
        with pytest.raises(ValueError, match="CUDA"):
            m.encode_reference(*R, lengths=torch.tensor(n_ref, device=DEV))


def test_auto_precision_gives_nan_only_where_the_reference_would():
    m, _ = _model(dict(variant="ViT-B16"), "auto")
    n_ref, n_dist, index = [8, 63], [63, 64, 8], [1, 0, 0]
    refs = _images(m.spec, n_ref, 700)
    dists = _images(m.spec, n_dist, 800, like=(refs, index))
    R, D = _cat(refs), _cat(dists)
    with torch.no_grad():
        q = m.forward_group(*_group_args(R, D), index, lengths=(n_ref, n_dist))[0]
        bad = D[0].clone()
        bad[63:63 + 64] = float("nan")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            qn = m.forward_group(*_group_args(R, (bad, D[1], D[2])), index, lengths=(n_ref, n_dist))[0]
        assert any("non-finite" in str(x.message) for x in w)
        assert m.engine_precision == "fp16x3"
        assert bool(torch.isnan(qn[1])) and torch.equal(bits32(qn[[0, 2]]), bits32(q[[0, 2]]))
        bad_pos = D[1].clone()
        bad_pos[70, 0] = -0.25
        with pytest.raises(IndexError):
            m.forward_group(*_group_args(R, (D[0], bad_pos, D[2])), index, lengths=(n_ref, n_dist))


# ---- 3: the C ABI: refusals that need a handle, footprint, reserve ---------------------------------------------------------------------
def _abi_calls(m, n_ref, n_dist, index, p):
    """The three entries on device pointers p(name): closures (group, encode, cached) over one engine."""
    lib, eng = m._engine_lib(), m._engine
    G, M = len(n_ref), len(n_dist)
    nr, nd, idx = (C.c_int32 * G)(*n_ref), (C.c_int32 * M)(*n_dist), (C.c_int32 * M)(*index)
    group = lambda: lib.vtq_forward_group_varlen(eng, p("patches0"), p("patches1"), p("pos0"), p("pos1"), p("scales0"), p("scales1"), G, M, nr, nd, idx,
                                                 p("q"), stream())
    encode = lambda: lib.vtq_encode_reference_varlen(eng, p("patches0"), p("pos0"), p("scales0"), G, nr, p("rows"), stream())
    cached = lambda: lib.vtq_forward_cached_varlen(eng, p("rows"), G, p("patches1"), p("pos1"), p("scales1"), M, nd, idx, p("qc"), stream())
    return group, encode, cached


def test_the_entries_keep_to_the_callers_tensors_and_refuse_a_trace():
    m, _ = _model(dict(variant="ViT-B16", num_scales=3), "fp16x3")
    n_ref, n_dist, index = [8, 63, 64], [64, 8, 45, 63, 1], [2, 0, 1, 1, 0]
    refs = _images(m.spec, n_ref, 900)
    dists = _images(m.spec, n_dist, 950, like=(refs, index))
    R, D = _cat(refs), _cat(dists)
    H = m.spec.hidden_size
    with torch.no_grad():                                                       # the ordinary calls (they also create the engine)
        q_ref = m.forward_group(*_group_args(R, D), index, lengths=(n_ref, n_dist))[0]
        rows_ref = m.encode_reference(*R, lengths=n_ref).rows
    torch.cuda.synchronize()
    L = Layout()
    for i, total in enumerate((sum(n_ref), sum(n_dist))):
        L.add(f"patches{i}", (total, 3, 16, 16), F32, 16 * 4), L.add(f"pos{i}", (total, 2), F32), L.add(f"scales{i}", (total,), F32)
    L.add("q", (len(n_dist),), F32), L.add("qc", (len(n_dist),), F32), L.add("rows", (len(n_ref), H), F32)
    a, v = L.build()
    for i, X in enumerate((R, D)):
        v[f"patches{i}"].copy_(X[0]), v[f"pos{i}"].copy_(X[1]), v[f"scales{i}"].copy_(X[2])
    group, encode, cached = _abi_calls(m, n_ref, n_dist, index, lambda n: v[n].data_ptr())
    lib, eng = m._engine_lib(), m._engine

    def launch():
        for call in (group, encode, cached):                                    # cached reads the rows encode has just written
            _lib.check(call())
    got_q, got_qc, got_rows = a.run_twice(launch, lambda: [v["q"], v["qc"], v["rows"]],
                                          prepare=lambda: (v["q"].zero_(), v["qc"].zero_(), v["rows"].zero_()))
    assert bool(torch.isfinite(got_q).all()) and torch.equal(bits32(got_q), bits32(q_ref))
    assert torch.equal(bits32(got_qc), bits32(q_ref)) and torch.equal(bits32(got_rows), bits32(rows_ref))
    flags = C.c_int32(-1)
    _lib.check(lib.vtq_input_errors(eng, C.byref(flags), stream()))
    assert flags.value == 0
    # a set token trace buffer: refused by name, nothing launched (the outputs keep their zeros)
    trace = torch.empty(3 * 16 * H, device=DEV)
    _lib.check(lib.vtq_set_token_trace(eng, trace.data_ptr()))
    try:
        for call, name, out in ((group, b"vtq_forward_group_varlen", "q"), (encode, b"vtq_encode_reference_varlen", "rows"),
                                (cached, b"vtq_forward_cached_varlen", "qc")):
            v[out].zero_()
            assert call() != 0
            assert name in lib.vtq_last_error() and b"trace" in lib.vtq_last_error()
            torch.cuda.synchronize()
            assert not bool(v[out].any())
    finally:
        _lib.check(lib.vtq_set_token_trace(eng, None))
    # scales are required by this model: NULL is refused as in vtq_forward
    nr, nd, idx = (C.c_int32 * 3)(*n_ref), (C.c_int32 * 5)(*n_dist), (C.c_int32 * 5)(*index)
    p = lambda n: v[n].data_ptr()
    assert lib.vtq_forward_group_varlen(eng, p("patches0"), p("patches1"), p("pos0"), p("pos1"), p("scales0"), None, 3, 5, nr, nd, idx, p("q"), stream()) != 0
    assert b"scales" in lib.vtq_last_error()
    assert lib.vtq_forward_group_varlen(eng, p("patches0"), None, p("pos0"), p("pos1"), p("scales0"), p("scales1"), 3, 5, nr, nd, idx, p("q"), stream()) != 0
    assert b"vtq_forward_group_varlen: null tensor" in lib.vtq_last_error()
    assert lib.vtq_forward_cached_varlen(eng, p("rows"), 3, p("patches1"), p("pos1"), p("scales1"), 5, nd, idx, None, stream()) != 0
    assert b"vtq_forward_cached_varlen: null output" in lib.vtq_last_error()


def test_reserve_means_no_call_allocates():
    m, _ = _model(dict(variant="ViT-B16"), "fp16x3")
    n_ref, n_dist, index, refs, dists = _data(m.spec, "plain", seed=1000)
    R, D = _cat(refs), _cat(dists)
    G, M, nmax = len(n_ref), len(n_dist), max(n_ref + n_dist)
    tiny = _images(m.spec, [4], 1)
    with torch.no_grad():
        m.encode_reference(*_cat(tiny), lengths=[4])                            # creates the engine and a small workspace
    lib, eng = m._engine_lib(), m._engine
    torch.cuda.synchronize()
    B = (G + M + 1) // 2
    _lib.check(lib.vtq_reserve(eng, B, nmax))

    def buffers():
        x, ln, big, rows = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(lib.vtq_debug_buffers(eng, C.byref(x), C.byref(ln), C.byref(big), C.byref(rows)))
        return x.value, ln.value, big.value, rows.value
    before, bytes_before = buffers(), lib.vtq_workspace_bytes(eng, B, nmax)
    rows = torch.empty(G, m.spec.hidden_size, device=DEV)
    q, qc = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    t = dict(patches0=R[0], pos0=R[1], scales0=None, patches1=D[0], pos1=D[1], scales1=None, rows=rows, q=q, qc=qc)
    group, encode, cached = _abi_calls(m, n_ref, n_dist, index, lambda n: None if t[n] is None else t[n].data_ptr())
    for call in (group, encode, cached, group):
        _lib.check(call())
        assert buffers() == before
    torch.cuda.synchronize()
    assert lib.vtq_workspace_bytes(eng, B, nmax) == bytes_before
    assert torch.equal(bits32(q), bits32(qc)) and bool(torch.isfinite(q).all())


# ---- 4: back to back on one engine, side streams, workspace growth ---------------------------------------------------------------------
def _calls(spec):
    """name -> closure(model) -> output tensor: the calls that share the engine's table with the ragged entries, and those entries."""
    n_ref, n_dist, index, refs, dists = _data(spec, "plain", seed=1100)
    R, D = _cat(refs), _cat(dists)
    G, M, N, uindex = 3, 7, 50, [2, 0, 0, 1, 2, 2, 0]
    U = tuple(tuple(None if t is None else t.to(DEV) for t in x) for x in _group(spec, G, M, N, uindex))
    return {
        "ragged_group": lambda m: m.forward_group(*_group_args(R, D), index, lengths=(n_ref, n_dist))[0],
        "uniform_group": lambda m: m.forward_group(*U, uindex)[0],
        "varlen": lambda m: m.forward_varlen((R[0], R[0].flip(0)), (R[1], R[1]), (None, None), n_ref)[0],      # the references, paired with themselves reversed
        "forward": lambda m: m((U[0][0], U[0][0].flip(1)), (U[1][0], U[1][0]), (None, None))[0],
        "ragged_cached": lambda m, ref=None: m.forward_cached(ref, *D, index, lengths=n_dist)[0],
        "ragged_encode": lambda m: m.encode_reference(*R, lengths=n_ref),
        "small_ragged_group": lambda m: m.forward_group(*_group_args(_cat(refs[:2]), _cat(dists[:2])), index[:2], lengths=(n_ref[:2], n_dist[:2]))[0],
    }


@pytest.fixture(scope="module")
def fresh_outputs(plain):
    """Every call of _calls on an engine of its own: what the same call has to give wherever it runs."""
    calls = _calls(plain.spec)
    out = {}
    with torch.no_grad():
        for name, call in calls.items():
            m, _ = _model(dict(variant="ViT-B16"), "fp16x3")
            if name == "ragged_cached":
                ref = calls["ragged_encode"](m)
                out[name] = call(m, ref)
            elif name == "ragged_encode":
                out[name] = call(m).rows
            else:
                out[name] = call(m)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pair", [("ragged_group", "uniform_group"), ("ragged_group", "varlen"), ("ragged_cached", "forward")])
@pytest.mark.parametrize("order", ["ab", "ba"])
def test_back_to_back_calls_on_one_engine(fresh_outputs, pair, order):
    """No host synchronisation between the two calls (an explicit precision reads no flags): the second call's table upload must not
    overwrite a section the first call's kernels still read."""
    m, _ = _model(dict(variant="ViT-B16"), "fp16x3")
    calls = _calls(m.spec)
    names = pair if order == "ab" else pair[::-1]
    with torch.no_grad():
        ref = calls["ragged_encode"](m) if "ragged_cached" in names else None
        got = {n: (calls[n](m, ref) if n == "ragged_cached" else calls[n](m)) for n in names}
        again = {n: (calls[n](m, ref) if n == "ragged_cached" else calls[n](m)) for n in names}
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(bits32(got[n]), bits32(fresh_outputs[n])), (n, order)
        assert torch.equal(bits32(again[n]), bits32(fresh_outputs[n])), (n, order, "second round")


def test_side_stream_and_workspace_growth(fresh_outputs):
    m, _ = _model(dict(variant="ViT-B16"), "fp16x3")
    calls = _calls(m.spec)
    with torch.no_grad():
        small = calls["small_ragged_group"](m)                                  # a small batch first ...
        grown = calls["ragged_group"](m)                                        # ... then G + M and max n both exceed it: the workspace grows
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            q_side = calls["ragged_group"](m)
            rows_side = calls["ragged_encode"](m)
            qc_side = calls["ragged_cached"](m, rows_side)
            small_side = calls["small_ragged_group"](m)                         # back to back on the side stream: the table is re-uploaded
        side.synchronize()
    assert torch.equal(bits32(small), bits32(fresh_outputs["small_ragged_group"]))
    assert torch.equal(bits32(grown), bits32(fresh_outputs["ragged_group"]))
    assert torch.equal(bits32(q_side), bits32(fresh_outputs["ragged_group"]))
    assert torch.equal(bits32(rows_side.rows), bits32(fresh_outputs["ragged_encode"]))
    assert torch.equal(bits32(qc_side), bits32(fresh_outputs["ragged_cached"]))
    assert torch.equal(bits32(small_side), bits32(fresh_outputs["small_ragged_group"]))
