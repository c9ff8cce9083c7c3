"""forward_group / encode_reference / forward_cached on the GPU: M distorted images over G references, every reference encoded once.

The contract every test here turns on: q[m] has the BITS the model gives for the single pair (reference ref_index[m], distorted image m) -- a
score never depends on what else is in the batch, nor on whether its reference was encoded in the same call or cached earlier.  The oracle
comparisons beside the bit checks keep them from being vacuous (two equal wrong answers)."""
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
from tests.test_gpu_parity import TOL, gate
from vtamiq_amd import VTAMIQ, ReferenceFeatures, StaleReferenceError, _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
bits32 = lambda t: t.contiguous().view(torch.int32)
INDEX = [2, 0, 0, 1, 2, 2, 0]                                  # G = 3, M = 7

# name -> (vit_config, engine options, G, M, ref_index)
CONFIGS = {
    "plain": (dict(variant="ViT-B16"), 0, 3, 7, INDEX),
    "tokens8_layerscale": (dict(variant="ViT-B16", num_extra_tokens=8, use_layer_scale=True), 0, 3, 7, INDEX),
    "scales3": (dict(variant="ViT-B16", num_scales=3), 0, 3, 7, INDEX),
    "full_last_layer": (dict(variant="ViT-B16"), _lib.OPT_FULL_LAST_LAYER, 3, 7, INDEX),
    "adapters": (dict(variant="ViT-B16", num_adapters=2, use_layer_scale=True), 0, 3, 7, INDEX),
    "vit_l16": (dict(variant="ViT-L16"), 0, 2, 3, [1, 0, 1]),
}


def _kw(vit):
    return dict(vit_config=dict(num_keep_layers=2, pretrained=False, **vit), num_rgs=2, num_rcabs=2, ca_reduction=16)


def _model(vit, precision, options=0, seed=71):
    m = VTAMIQ(**json.loads(json.dumps(_kw(vit))), precision=precision, engine_options=options)
    sd = synth.make_state_dict(m.spec, seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval(), sd


def _group(spec, G, M, N, index, seed=300, N_dist=None, embedded=False):
    """CPU tensors of one group: ((p_ref, p_dist), (pos_ref, pos_dist), (sc_ref, sc_dist) | (None, None)).  The references are G images of
    synth.make_inputs; distorted image m is its reference plus noise (positions of its own), or an image of its own when N_dist != N."""
    pa, po, sc = synth.make_inputs(spec, G, N, seed, aligned=False)
    r = np.random.RandomState(seed + 1)
    Nd = N_dist or N
    if embedded:
        p_ref = (0.3 * r.normal(size=(G, N, spec.hidden_size))).astype(np.float32)
        p_dist = (p_ref[index] + 0.03 * r.normal(size=(M, N, spec.hidden_size))).astype(np.float32)
    elif Nd == N:
        p_ref = pa[:, 0]
        p_dist = np.clip(p_ref[index] + 0.1 * r.normal(size=(M, *p_ref.shape[1:])), -1.0, 1.0).astype(np.float32)
    else:
        p_ref = pa[:, 0]
        p_dist = r.uniform(-1.0, 1.0, size=(M, Nd, *p_ref.shape[2:])).astype(np.float32)
    pos_dist = np.minimum(r.uniform(0.0, 1.0, size=(M, Nd, 2)), 1.0 - 1e-6).astype(np.float32)
    t = torch.from_numpy
    scales = (None, None)
    if sc is not None:
        sd_ = synth.make_inputs(spec, M, Nd, seed, aligned=False)[2]
        scales = (t(sc[:, 0]).float(), t(sd_[:, 1]).float())
    return (t(p_ref), t(p_dist)), (t(po[:, 0]), t(pos_dist)), scales


def _dev(ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _pair(grp, i, m):
    """The single pair (reference i, distorted m) of a group, as forward() takes it."""
    return tuple((None if a is None else a[i:i + 1], None if b is None else b[m:m + 1]) for a, b in grp)


def _alone(model, grp, index):
    """M single-pair forward() calls: the bits every one-to-many entry has to give."""
    return torch.cat([model(*_pair(grp, i, m))[0] for m, i in enumerate(index)])


def _oracle(sd, spec, grp, index, token_num=0):
    """The reference forward (oracle, on the host) of every expanded pair."""
    (pr, pd), (qr, qd), (sr, sdist) = grp
    idx = torch.tensor(index)
    pick = lambda a: None if a is None else a[idx]
    return O.vtamiq_forward(O.to_torch(sd), spec, (pick(pr), pd), (pick(qr), qd), (pick(sr), sdist), token_num=token_num)[0].numpy()


@functools.lru_cache(maxsize=None)
def _oracle_scores(name):
    """Once per configuration, shared by the precisions."""
    vit, _, G, M, index = CONFIGS[name]
    m = VTAMIQ(**json.loads(json.dumps(_kw(vit))), precision="bf16")
    return _oracle(synth.make_state_dict(m.spec, 71), m.spec, _group(m.spec, G, M, 50, index), index)


# ---- 1: bits of the pair alone, plus the oracle gate ---------------------------------------------------------------------------------
def _e2e(name, precision):
    vit, options, G, M, index = CONFIGS[name]
    m, _ = _model(vit, precision, options)
    grp = tuple(_dev(x) for x in _group(m.spec, G, M, 50, index))
    with torch.no_grad():
        q, aux = m.forward_group(*grp, index)
        alone = _alone(m, grp, index)
        again = m.forward_group(*grp, torch.tensor(index))[0]        # after the B = 1 calls, and with a CPU tensor
    assert aux is None and q.shape == (M,) and q.dtype == torch.float32 and bool(torch.isfinite(q).all())
    assert torch.equal(bits32(q), bits32(alone)), (q - alone).abs().max().item()
    assert torch.equal(bits32(q), bits32(again))
    m.check_inputs()
    ref = _oracle_scores(name)
    e = rel_err(q.cpu().numpy(), ref)
    print(f"\n[group {name} {precision}] {e}")
    assert gate(q.cpu().numpy(), ref, TOL[precision]), e


@pytest.mark.parametrize("precision", ["fp16x3", "fp16x2", "bf16"])
@pytest.mark.parametrize("name", ["plain", "tokens8_layerscale", "scales3", "full_last_layer", "adapters"])
def test_scores_have_the_bits_of_the_pair_alone(name, precision):
    _e2e(name, precision)


def test_scores_have_the_bits_of_the_pair_alone_vit_l16():
    _e2e("vit_l16", "fp16x3")


def test_last_register_token_and_pre_embedded_input():
    """token_num = -1 on the register-token model (the last register token feeds the head), and pre-embedded (G | M, N, H) rows."""
    vit, _, G, M, index = CONFIGS["tokens8_layerscale"]
    m, sd = _model(vit, "fp16x3")
    m.token_num = -1
    cpu = _group(m.spec, G, M, 50, index)
    grp = tuple(_dev(x) for x in cpu)
    with torch.no_grad():
        q = m.forward_group(*grp, index)[0]
        alone = _alone(m, grp, index)
    assert torch.equal(bits32(q), bits32(alone))
    ref = _oracle(sd, m.spec, cpu, index, token_num=m.spec.num_tokens - 1)
    assert gate(q.cpu().numpy(), ref, TOL["fp16x3"]), rel_err(q.cpu().numpy(), ref)
    m.token_num = 0
    with torch.no_grad():
        q0 = m.forward_group(*grp, index)[0]
    assert not torch.equal(bits32(q0), bits32(q))                        # the token is read at every call
    cpu = _group(m.spec, G, M, 50, index, embedded=True)
    grp = tuple(_dev(x) for x in cpu)
    with torch.no_grad():
        q = m.forward_group(*grp, index)[0]
        alone = _alone(m, grp, index)
        ref_f = m.encode_reference(grp[0][0], grp[1][0])
        qc = m.forward_cached(ref_f, grp[0][1], grp[1][1], None, index)[0]
    assert torch.equal(bits32(q), bits32(alone)) and torch.equal(bits32(qc), bits32(alone))
    ref = _oracle(sd, m.spec, cpu, index)
    assert gate(q.cpu().numpy(), ref, TOL["fp16x3"]), rel_err(q.cpu().numpy(), ref)


# ---- 2: shapes where the layout can go wrong ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    return _model(dict(variant="ViT-B16"), "fp16x3")


SHAPES = {
    "odd_sequence_count": (2, 3, 50, [1, 0, 1]),
    "S128_query_block_boundary": (2, 3, 127, [0, 1, 1]),
    "S131_one_past_the_boundary": (2, 3, 130, [1, 1, 0]),
    "one_pair": (1, 1, 50, [0]),
    "unused_reference": (3, 4, 50, [2, 0, 0, 2]),
    "2048_rows_256_tile_gemms": (4, 12, 127, [3, 0, 1, 2, 2, 1, 0, 3, 3, 3, 0, 1]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_layout_shapes(plain, shape):
    m, sd = plain
    G, M, N, index = SHAPES[shape]
    cpu = _group(m.spec, G, M, N, index, seed=410)
    grp = tuple(_dev(x) for x in cpu)
    with torch.no_grad():
        q = m.forward_group(*grp, index)[0]
        alone = _alone(m, grp, index)
    assert torch.equal(bits32(q), bits32(alone)), (shape, (q - alone).abs().max().item())
    if shape == "one_pair":
        with torch.no_grad():
            assert torch.equal(bits32(q), bits32(m(*grp)[0]))                # forward() at B = 1
    if shape == "2048_rows_256_tile_gemms":
        lib = _lib.load()
        H, S = m.spec.hidden_size, N + m.spec.num_tokens
        big, small = (G + M) * S, -(-2 * S // 256) * 256
        assert big == 2048                                                   # the group takes the 256x256 form, a pair alone a small tile
        assert lib.vtq_k_gemm_tile_rule(big, 3 * H, H, _lib.NUM["fp16x3"]) == 0 != lib.vtq_k_gemm_tile_rule(small, 3 * H, H, _lib.NUM["fp16x3"])
    ref = _oracle(sd, m.spec, cpu, index)
    assert gate(q.cpu().numpy(), ref, TOL["fp16x3"]), rel_err(q.cpu().numpy(), ref)


# ---- 3: equivalence with the existing entry points ----------------------------------------------------------------------------------
def test_pairwise_forward_and_permutations(plain):
    m, _ = plain
    N = 50
    pa, po, _ = synth.make_inputs(m.spec, 5, N, 12, aligned=False)
    t = lambda a: torch.from_numpy(a).to(DEV)
    pr, pd, qr, qd = t(pa[:, 0]), t(pa[:, 1]), t(po[:, 0]), t(po[:, 1])
    d2 = (pd + 0.05).clamp(-1, 1)
    with torch.no_grad():
        # forward_pairwise on B = 3: (ref, dist1), (ref, dist2)
        q1, q2 = m.forward_pairwise((pr[:3], pd[:3], d2[:3]), (qr[:3], qd[:3], qd[:3]), None)
        qg = m.forward_group((pr[:3], torch.cat([pd[:3], d2[:3]])), (qr[:3], torch.cat([qd[:3], qd[:3]])), (None, None), [0, 1, 2, 0, 1, 2])[0]
        assert torch.equal(bits32(qg), bits32(torch.cat([q1, q2])))
        # forward on B = 5
        q = m((pr, pd), (qr, qd), (None, None))[0]
        qg = m.forward_group((pr, pd), (qr, qd), (None, None), range(5))[0]
        assert torch.equal(bits32(qg), bits32(q))
        # permuting the distorted images and ref_index together permutes the bits
        index, perm = [4, 0, 0, 3, 1], [3, 0, 4, 2, 1]
        qa = m.forward_group((pr, pd), (qr, qd), (None, None), index)[0]
        qp = m.forward_group((pr, pd[perm]), (qr, qd[perm]), (None, None), [index[i] for i in perm])[0]
    assert torch.equal(bits32(qp), bits32(qa[perm]))


# ---- 4: the cache -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "full_last_layer", "adapters"])
def test_cached_scores_have_the_bits_of_the_group(name):
    vit, options, G, M, index = CONFIGS[name]
    m, _ = _model(vit, "fp16x3", options)
    (pr, pd), (qr, qd), (sr, sdist) = (_dev(x) for x in _group(m.spec, G, M, 50, index))
    with torch.no_grad():
        q = m.forward_group((pr, pd), (qr, qd), (sr, sdist), index)[0]
        ref = m.encode_reference(pr, qr, sr)
        assert isinstance(ref, ReferenceFeatures) and ref.rows.shape == (G, m.spec.hidden_size) and ref.rows.dtype == F32
        assert (ref.precision, ref.token, ref.engine_options) == ("fp16x3", 0, options) and len(ref) == G
        qc = m.forward_cached(ref, pd, qd, sdist, index)[0]
        assert torch.equal(bits32(qc), bits32(q))
        # two chunks, with a much larger forward between them: the workspace grows and is reused, the rows are the caller's
        qa = m.forward_cached(ref, pd[:3], qd[:3], None if sdist is None else sdist[:3], index[:3])[0]
        big = synth.make_inputs(m.spec, 32, 200, 5)
        tb = lambda a, i: None if a is None else torch.from_numpy(a[:, i]).float().to(DEV)
        m((tb(big[0], 0), tb(big[0], 1)), (tb(big[1], 0), tb(big[1], 1)), (tb(big[2], 0), tb(big[2], 1)))
        qb = m.forward_cached(ref, pd[3:], qd[3:], None if sdist is None else sdist[3:], index[3:])[0]
        assert torch.equal(bits32(torch.cat([qa, qb])), bits32(q))
        # references encoded in two calls and concatenated
        two = ReferenceFeatures.cat([m.encode_reference(pr[:1], qr[:1], None if sr is None else sr[:1]),
                                     m.encode_reference(pr[1:], qr[1:], None if sr is None else sr[1:])])
        assert torch.equal(bits32(two.rows), bits32(ref.rows))
        assert torch.equal(bits32(m.forward_cached(two, pd, qd, sdist, index)[0]), bits32(q))
        # ref_index=None: distorted image m against reference m
        qn = m.forward_cached(ref, pd[:G], qd[:G], None if sdist is None else sdist[:G])[0]
        assert torch.equal(bits32(qn), bits32(m((pr, pd[:G]), (qr, qd[:G]), (sr, None if sdist is None else sdist[:G]))[0]))
    m.check_inputs()


def test_cached_other_patch_count_and_side_stream(plain):
    """Distorted images of N = 77 against references of N = 50: nothing behind the encoder depends on N.  No single forward() takes such a
    pair, so the gate is the oracle's head on the two token sets; then the same call on a side stream."""
    m, sd = plain
    G, M, index = 3, 7, INDEX
    cpu = _group(m.spec, G, M, 50, index, seed=520, N_dist=77)
    (pr, pd), (qr, qd), _ = (_dev(x) for x in cpu)
    with torch.no_grad():
        ref = m.encode_reference(pr, qr)
        q = m.forward_cached(ref, pd, qd, None, index)[0]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            q_side = m.forward_cached(ref, pd, qd, None, index)[0]
            q_side2 = m.forward_cached(ref, pd[:2], qd[:2], None, index[:2])[0]      # back to back: ref_index is uploaded again
        side.synchronize()
    assert torch.equal(bits32(q_side), bits32(q)) and torch.equal(bits32(q_side2), bits32(q[:2]))
    sdt = O.to_torch(sd)
    (cr, cd), (cqr, cqd), _ = cpu
    with torch.no_grad():
        want = O.head(sdt, m.spec, O.vit_tokens(sdt, m.spec, cr, cqr, None)[torch.tensor(index)], O.vit_tokens(sdt, m.spec, cd, cqd, None)).numpy()
    assert gate(q.cpu().numpy(), want, TOL["fp16x3"]), rel_err(q.cpu().numpy(), want)


# ---- 5: a stale cache is never scored -----------------------------------------------------------------------------------------------
def test_stale_references_are_refused():
    vit = dict(variant="ViT-B16", num_extra_tokens=2)
    m, sd = _model(vit, "fp16x3")
    G, M, index = 3, 7, INDEX
    (pr, pd), (qr, qd), _ = (_dev(x) for x in _group(m.spec, G, M, 50, index))
    with torch.no_grad():
        ref = m.encode_reference(pr, qr)
        q = m.forward_cached(ref, pd, qd, None, index)[0]
    torch.cuda.synchronize()
    flags0 = m._read_flags()

    def refused(model=m):
        with pytest.raises(ValueError) as ei, torch.no_grad():
            model.forward_cached(ref, pd, qd, None, index)
        assert isinstance(ei.value, StaleReferenceError)

    m.precision = "fp16x2"
    refused()
    m.precision = "fp16x3"
    m.token_num = 1
    refused()
    m.token_num = -3                                                      # resolves to token 0 of 3: the same token, not stale
    with torch.no_grad():
        assert torch.equal(bits32(m.forward_cached(ref, pd, qd, None, index)[0]), bits32(q))
    m.token_num = 0
    m.engine_options = _lib.OPT_FULL_LAST_LAYER
    refused()
    m.engine_options = 0
    other, _ = _model(vit, "fp16x3")                                      # the same weights in another model, on another engine
    refused(other)
    with torch.no_grad():
        assert torch.equal(bits32(m.forward_cached(ref, pd, qd, None, index)[0]), bits32(q))       # every attribute restored: valid again
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})   # the same values: still a reload
    refused()
    assert m._read_flags() == flags0 == 0
    with torch.no_grad():
        ref2 = m.encode_reference(pr, qr)
        assert torch.equal(bits32(m.forward_cached(ref2, pd, qd, None, index)[0]), bits32(q))


def test_auto_overflow_during_forward_cached():
    """precision="auto": the LayerNorm gain of one channel is scaled so that ONE distorted image -- the one with a patch that lies along that
    channel's patch-embedding row, whose normalised row is peaked there -- leaves the fp16 range, and nothing else does.  The references encode
    in fp16x3; forward_cached on the batch with that image switches the model to bf16x3 and raises; after re-encoding the scores are
    finite and inside the bf16x3 gate."""
    m = VTAMIQ(**json.loads(json.dumps(_kw(dict(variant="ViT-B16")))))
    assert m.precision == "auto"
    spec = m.spec
    sd = synth.make_state_dict(spec, 71)
    G, M, index = 3, 7, INDEX
    cpu = _group(spec, G, M, 50, index, seed=630)
    (cr, cd), (cqr, cqd), _ = cpu
    w0 = torch.from_numpy(sd["transformer.embeddings.patch_embeddings.weight"])[0]
    cd[4, 9] = 300.0 * torch.sign(w0)                                    # image 4, patch 9: along output channel 0
    sdt = O.to_torch(sd)
    lw, lb = sdt["transformer.encoder.layers.0.attention_norm.weight"], sdt["transformer.encoder.layers.0.attention_norm.bias"]
    ch0 = lambda p, q: (O._layer_norm(O.embeddings(sdt, spec, p, q, None), lw, lb)[..., 0] / lw[0]).abs()
    a_ref, a_dist = ch0(cr, cqr), ch0(cd, cqd)
    a_peak = float(a_dist[4].max())
    a_dist[4, a_dist[4].argmax()] = 0.0
    a_rest = max(float(a_ref.max()), float(a_dist.max()))
    assert a_peak > 3.0 * a_rest, (a_peak, a_rest)                       # the construction: one row stands out
    gain = 65504.0 / (0.5 * (a_peak + a_rest))                           # peak * gain > 65504 > rest * gain, with the same margin both ways
    sd["transformer.encoder.layers.0.attention_norm.weight"][0] *= gain / float(lw[0])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).eval()
    (pr, pd), (qr, qd), _ = (_dev(x) for x in cpu)
    with torch.no_grad():
        ref = m.encode_reference(pr, qr)
        assert m.engine_precision == "fp16x3" and ref.precision == "fp16x3"
        keep = [i for i in range(M) if i != 4]
        q_ok = m.forward_cached(ref, pd[keep], qd[keep], None, [index[i] for i in keep])[0]
        assert m.engine_precision == "fp16x3" and bool(torch.isfinite(q_ok).all())
        with warnings.catch_warnings(record=True) as w, pytest.raises(StaleReferenceError):
            warnings.simplefilter("always")
            m.forward_cached(ref, pd, qd, None, index)
        assert any("bf16x3" in str(x.message) for x in w) and m.engine_precision == "bf16x3"
        with pytest.raises(ValueError):
            m.forward_cached(ref, pd, qd, None, index)                   # still the fp16x3 rows
        ref = m.encode_reference(pr, qr)
        q = m.forward_cached(ref, pd, qd, None, index)[0]
    assert ref.precision == "bf16x3" and bool(torch.isfinite(q).all())
    want = _oracle(sd, spec, cpu, index)
    e = rel_err(q.cpu().numpy(), want)
    print(f"\n[auto -> bf16x3 during forward_cached] {e}")
    assert gate(q.cpu().numpy(), want, TOL["bf16x3"]), e


# ---- 6: input policy ----------------------------------------------------------------------------------------------------------------
def test_input_policy(plain):
    m, _ = plain
    G, M, index = 3, 7, INDEX
    (pr, pd), (qr, qd), sc = (_dev(x) for x in _group(m.spec, G, M, 50, index, seed=600))
    with torch.no_grad():
        q = m.forward_group((pr, pd), (qr, qd), sc, index)[0]
        m.check_inputs()
        bad = qr.clone()
        bad[1, 5, 1] = 1.5                                               # a reference's position
        m.forward_group((pr, pd), (bad, qd), sc, index)
        with pytest.raises(IndexError):
            m.check_inputs()
        bad = qd.clone()
        bad[6, 49, 0] = -0.25                                            # a distorted image's
        m.forward_group((pr, pd), (qr, bad), sc, index)
        with pytest.raises(IndexError):
            m.check_inputs()
        bad_d = pd.clone()
        bad_d[3] = float("nan")
        qn = m.forward_group((pr, bad_d), (qr, qd), sc, index)[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        keep = [i for i in range(M) if i != 3]
        assert bool(torch.isnan(qn[3])) and torch.equal(bits32(qn[keep]), bits32(q[keep]))
        bad_r = pr.clone()
        bad_r[2, 7, 1, 3, 3] = float("nan")
        qn = m.forward_group((bad_r, pd), (qr, qd), sc, index)[0]
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        hit = [i for i in range(M) if index[i] == 2]
        keep = [i for i in range(M) if index[i] != 2]
        assert bool(torch.isnan(qn[hit]).all()) and torch.equal(bits32(qn[keep]), bits32(q[keep]))
        m.encode_reference(bad_r, qr)
        with pytest.raises(FloatingPointError):
            m.check_inputs()
        m.encode_reference(pr, qr)
        m.check_inputs()
        with pytest.raises(ValueError, match="CUDA"):
            m.forward_group((pr, pd), (qr, qd), sc, torch.tensor(index, device=DEV))
        with pytest.raises(ValueError, match="ref_index"):
            m.forward_group((pr, pd), (qr, qd), sc, index[:-1] + [3])
        assert torch.equal(bits32(m.forward_group((pr, pd), (qr, qd), sc, index)[0]), bits32(q))


# ---- 7: footprint -------------------------------------------------------------------------------------------------------------------
def test_the_c_entries_keep_to_the_callers_tensors():
    m, _ = _model(dict(variant="ViT-B16", num_scales=3), "fp16x3")
    G, M, N, index = 2, 3, 50, [1, 0, 1]
    H = m.spec.hidden_size
    (pr, pd), (qr, qd), (sr, sdist) = (_dev(x) for x in _group(m.spec, G, M, N, index, seed=900))
    with torch.no_grad():
        q_ref = m.forward_group((pr, pd), (qr, qd), (sr, sdist), index)[0]   # the ordinary call (it also creates the engine)
        rows_ref = m.encode_reference(pr, qr, sr).rows
    torch.cuda.synchronize()
    L = Layout()
    for name, n in (("ref", G), ("dist", M)):
        L.add(f"patches_{name}", (n, N, 3, 16, 16), F32, 16 * 4), L.add(f"pos_{name}", (n, N, 2), F32), L.add(f"scales_{name}", (n, N), F32)
    L.add("ref_rows", (G, H), F32)
    L.add("q", (M,), F32)
    a, v = L.build()
    for name, (pt, po, sc) in (("ref", (pr, qr, sr)), ("dist", (pd, qd, sdist))):
        v[f"patches_{name}"].copy_(pt), v[f"pos_{name}"].copy_(po), v[f"scales_{name}"].copy_(sc)
    lib, eng = m._engine_lib(), m._engine
    p = lambda n: v[n].data_ptr()
    arr = (C.c_int32 * M)(*index)
    group = lambda ix, g=G: lib.vtq_forward_group(eng, p("patches_ref"), p("patches_dist"), p("pos_ref"), p("pos_dist"), p("scales_ref"), p("scales_dist"),
                                                  g, M, N, ix, p("q"), stream())
    encode = lambda g=G: lib.vtq_encode_reference(eng, p("patches_ref"), 0, p("pos_ref"), p("scales_ref"), g, N, p("ref_rows"), stream())
    cached = lambda ix, n=N: lib.vtq_forward_cached(eng, p("ref_rows"), G, p("patches_dist"), 0, p("pos_dist"), p("scales_dist"), M, n, ix, p("q"), stream())
    (got,) = a.run_twice(lambda: _lib.check(group(arr)), lambda: [v["q"]], prepare=lambda: v["q"].zero_())
    assert bool(torch.isfinite(got).all()) and torch.equal(bits32(got), bits32(q_ref))
    (rows,) = a.run_twice(lambda: _lib.check(encode()), lambda: [v["ref_rows"]], prepare=lambda: v["ref_rows"].zero_())
    assert bool(torch.isfinite(rows).all()) and torch.equal(bits32(rows), bits32(rows_ref))
    v["ref_rows"].copy_(rows)
    (got,) = a.run_twice(lambda: _lib.check(cached(arr)), lambda: [v["q"]], prepare=lambda: v["q"].zero_())
    assert torch.equal(bits32(got), bits32(q_ref))
    # calls refused for a bad argument launch nothing: outputs and guards keep the fill
    bad = (C.c_int32 * M)(1, 2, 0)
    for byte in (0x00, 0xFF):
        a.fill_guards(byte)
        a.fill(v["q"], byte), a.fill(v["ref_rows"], byte)
        for call in (lambda: group(bad), lambda: group(None), lambda: group(arr, 0), lambda: encode(0), lambda: cached(bad), lambda: cached(arr, 0)):
            assert call() != 0 and lib.vtq_last_error()
        torch.cuda.synchronize()
        assert not a.violations(byte)
        assert bool((v["q"].view(torch.uint8) == byte).all()) and bool((v["ref_rows"].view(torch.uint8) == byte).all())
    flags = C.c_int32(-1)
    _lib.check(lib.vtq_input_errors(eng, C.byref(flags), stream()))
    assert flags.value == 0
