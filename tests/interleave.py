"""Every public forward entry as a named call, a plan that runs them in every order, and the comparison with a fresh engine.

The engine (vtamiq_amd/csrc/engine.hip) is state shared by all calls on one handle: a workspace that only grows and is zero-filled only
when it is allocated, a second one for forward_rollout, the settings the ABI keeps between calls (trace, iqa_token), one device table
(vl_tab) used by forward_varlen and by the group / cached entries.  tests/test_gpu_interleave.py and tests/test_gpu_streams.py
run the calls of this catalogue back to back on one model and compare every output, bit for bit, with the same call on a model that has
run nothing else (`reference`).  tests/test_interleave_plan.py checks, without a GPU, what those tests rely on: that the plan holds every
ordered pair of kinds, and that a poisoned carrier call covers the slack rows of every clean call that follows it.

Importing this module needs no GPU; tensors reach the device when a call is first used."""
import itertools
import json

import numpy as np
import torch

from vtamiq_amd import VTAMIQ, synth
from vtamiq_amd.spec import make_spec

DEV = "cuda"
# two layers, T = 2 tokens (CLS + one register token, so token_num can change), a small head: a call takes about a millisecond
KW = dict(vit_config=dict(variant="ViT-B16", num_keep_layers=2, num_extra_tokens=1, pretrained=False), num_rgs=2, num_rcabs=2, ca_reduction=16)
WSEED = 501
T = 2


def spec():
    return make_spec(**json.loads(json.dumps(KW)))


# ---- geometry: geometry_seq() of engine.hip on the host --------------------------------------------------------------------------------
def ceil256(rows):
    return (rows + 255) // 256 * 256


def seq_rows(nseq, N):
    """Token rows of nseq sequences of N patches, packed back to back: nseq * S."""
    return nseq * (N + T)


def varlen_rows(lengths):
    """Token rows of a forward_varlen call: both images of every pair at their own length."""
    return 2 * (sum(lengths) + len(lengths) * T)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def _noise(seed, shape, scale):
    return (scale * np.random.RandomState(seed).normal(size=shape)).astype(np.float32)


def _pos(seed, *shape):
    return np.minimum(np.random.RandomState(seed).uniform(0.0, 1.0, size=(*shape, 2)), 1.0 - 1e-6).astype(np.float32)


class Entry:
    """One named call.  kind: which public entry; size: "small" | "large"; rows: token rows of each engine call it makes (one, or two for
    encode_reference -> forward_cached); pair_axes: per output tensor, the axis that indexes the call's images / pairs (what a NaN in one
    image may touch); offsets: forward_varlen only, the first patch row of every pair."""

    def __init__(self, name, kind, size, rows, seed, make, call, pair_axes, offsets=None):
        self.name, self.kind, self.size, self.rows, self.seed = name, kind, size, list(rows), seed
        self._make, self._call, self.pair_axes, self.offsets = make, call, pair_axes, offsets
        self._inputs = None

    @property
    def m_pad(self):
        return max(ceil256(r) for r in self.rows)

    def inputs(self):
        """The call's seeded inputs on the device: made once, never modified (the poisoned variants are clones)."""
        if self._inputs is None:
            self._inputs = {k: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in v) for k, v in self._make(self.seed).items()}
        return self._inputs

    def run(self, model, inp=None):
        """-> tuple of the call's output tensors, as the model returns them (not cloned, not synchronised)."""
        with torch.no_grad():
            return tuple(self._call(model, inp if inp is not None else self.inputs()))

    def poisoned(self, value, every_image):
        """A clone of the inputs with one sample of EVERY image set to `value` (every_image), or of the image with index 1 of the last
        patch tensor only (the distorted image of pair 1; for forward_vit, image 1)."""
        inp = {k: tuple(t.clone() for t in v) for k, v in self.inputs().items()}
        tensors = inp["p"] if every_image else inp["p"][-1:]
        for t in tensors:
            if self.offsets is not None:                       # varlen: (sum(lengths), 3, P, P), pair b from row offsets[b]
                for b in (range(len(self.offsets)) if every_image else [1]):
                    t[self.offsets[b] + 1, 1, 3, 3] = value
            else:
                for b in (range(t.shape[0]) if every_image else [1]):
                    t[b, 7, 1, 3, 3] = value
        return inp


def _pairs(B, N):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), B, N, seed)
        return dict(p=(pa[:, 0], pa[:, 1]), pos=(po[:, 0], po[:, 1]))
    return make


def _rows_pairs(B, N):
    def make(seed):
        ref = _noise(seed, (B, N, 768), 0.3)
        return dict(p=(ref, ref + _noise(seed + 1, ref.shape, 0.03)), pos=(_pos(seed + 2, B, N),) * 2)
    return make


def _triplets(B, N):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), B, N, seed)
        d2 = np.clip(pa[:, 0] + _noise(seed + 1, pa[:, 0].shape, 0.2), -1.0, 1.0)
        return dict(p=(pa[:, 0], pa[:, 1], d2), pos=(po[:, 0], po[:, 1], po[:, 1]))
    return make


def _singles(B, N):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), B, N, seed)
        return dict(p=(pa[:, 0],), pos=(po[:, 0],))
    return make


def _varlen(lengths):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), 1, sum(lengths), seed)
        return dict(p=(pa[0, 0], pa[0, 1]), pos=(po[0, 0], po[0, 1]))
    return make


def _group(G, M, N, index):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), G, N, seed)
        dist = np.clip(pa[:, 0][index] + _noise(seed + 1, (M, *pa.shape[2:]), 0.1), -1.0, 1.0)
        return dict(p=(pa[:, 0], dist), pos=(po[:, 0], _pos(seed + 2, M, N)))
    return make


def _cached(G, N, M, N2):
    def make(seed):
        pa, po, _ = synth.make_inputs(spec(), G, N, seed)
        pd, qd, _ = synth.make_inputs(spec(), M, N2, seed + 1)
        return dict(p=(pa[:, 0], pd[:, 1]), pos=(po[:, 0], qd[:, 1]))
    return make


def _call_forward(m, i):
    return (m(i["p"], i["pos"], None)[0],)


def _call_pairwise(m, i):
    return m.forward_pairwise(i["p"], i["pos"], None)


def _call_rollout(m, i):
    q, r = m.forward_rollout(i["p"], i["pos"], None)
    return q, r.rollout, r.last_attention


def _call_vit(tokens_only, layers, attention):
    def call(m, i):
        enc = m.transformer.encoder
        enc.return_layers, enc.return_attention = layers, attention         # read by forward_vit at every call
        x, probs, states = m.forward_vit(i["p"][0], i["pos"][0], None, tokens_only=tokens_only)
        assert len(probs) == (2 if attention else 0) and len(states) == (2 if layers else 0)
        return (x, *probs, *states)
    return call


def _call_varlen(lengths):
    return lambda m, i: (m.forward_varlen(i["p"], i["pos"], None, lengths)[0],)


def _call_group(index):
    return lambda m, i: (m.forward_group(i["p"], i["pos"], None, index)[0],)


def _call_cached(index):
    def call(m, i):
        ref = m.encode_reference(i["p"][0], i["pos"][0], None)
        return ref.rows, m.forward_cached(ref, i["p"][1], i["pos"][1], None, index)[0]
    return call


def _offsets(lengths):
    return [int(v) for v in np.cumsum([0] + list(lengths[:-1]))]


# varlen, small: [8, 130, 110] and not [8, 130, 63] -- 508 rows, 4 short of M_pad = 512, so that the last sequence's second 64-key tile
# (rows 396 .. 523) reads the slack rows vtq_forward_varlen clears; with 63 the over-read ends at row 476, inside M_pad
VL_SMALL, VL_LARGE = [8, 130, 110], [300, 5, 40, 77]
GROUP_SMALL, GROUP_LARGE, CACHED_INDEX = [1, 0, 1], [0, 0, 0, 0], [1, 0, 1]
# forward_vit, large: B = 5 at N = 130 and not fewer images -- as a poison carrier its 660 rows must reach M_pad + 128 = 640 of the small
# varlen call (508 rows); that is 8.4 MB of attention maps per call
_ENTRIES = [
    Entry("forward_small", "forward", "small", [seq_rows(4, 40)], 1101, _pairs(2, 40), _call_forward, (0,)),
    Entry("forward_large", "forward", "large", [seq_rows(6, 300)], 1102, _pairs(3, 300), _call_forward, (0,)),
    Entry("forward_rows_small", "forward_rows", "small", [seq_rows(4, 40)], 1103, _rows_pairs(2, 40), _call_forward, (0,)),
    Entry("pairwise_small", "pairwise", "small", [seq_rows(6, 40)], 1104, _triplets(2, 40), _call_pairwise, (0, 0)),     # 252 rows: 4 short of the tile
    Entry("pairwise_large", "pairwise", "large", [seq_rows(6, 300)], 1105, _triplets(2, 300), _call_pairwise, (0, 0)),
    Entry("vit_small", "vit", "small", [seq_rows(3, 40)], 1106, _singles(3, 40), _call_vit(True, True, False), (0, 0, 0)),
    Entry("vit_large", "vit", "large", [seq_rows(5, 130)], 1107, _singles(5, 130), _call_vit(False, True, True), (0, 0, 0, 0, 0)),
    # rollout, small: B = 3 and not 2 -- 6 x 42 = 252 rows as the pairwise triplets, so that the last sequence's 64-key tile (rows 210 .. 273)
    # reads the slack rows of the ro_qkv buffers; at B = 2 (168 rows) every over-read ends inside M_pad.  (The kernels mask what they read
    # there by themselves: a stale NaN in those rows reaches no output even without the engine's memset, which is what the tests pin.)
    Entry("rollout_small", "rollout", "small", [seq_rows(6, 40)], 1108, _pairs(3, 40), _call_rollout, (0, 1, 1)),
    Entry("rollout_large", "rollout", "large", [seq_rows(6, 300)], 1109, _pairs(3, 300), _call_rollout, (0, 1, 1)),
    Entry("varlen_small", "varlen", "small", [varlen_rows(VL_SMALL)], 1110, _varlen(VL_SMALL), _call_varlen(VL_SMALL), (0,), _offsets(VL_SMALL)),
    Entry("varlen_large", "varlen", "large", [varlen_rows(VL_LARGE)], 1111, _varlen(VL_LARGE), _call_varlen(VL_LARGE), (0,), _offsets(VL_LARGE)),
    Entry("group_small", "group", "small", [seq_rows(5, 40)], 1112, _group(2, 3, 40, GROUP_SMALL), _call_group(GROUP_SMALL), (0,)),    # 5 sequences: odd
    Entry("group_large", "group", "large", [seq_rows(5, 300)], 1113, _group(1, 4, 300, GROUP_LARGE), _call_group(GROUP_LARGE), (0,)),
    Entry("cached_small", "cached", "small", [seq_rows(2, 40), seq_rows(3, 77)], 1114, _cached(2, 40, 3, 77), _call_cached(CACHED_INDEX), (None, 0)),
]
CATALOGUE = {e.name: e for e in _ENTRIES}
KINDS = tuple(dict.fromkeys(e.kind for e in _ENTRIES))                      # in catalogue order
SMALL = [e.name for e in _ENTRIES if e.size == "small"]                     # one call of every kind
# part b of tests/test_gpu_interleave.py: every image of a carrier holds one non-finite sample, then every SMALL call runs on that engine
CARRIERS = ["forward_large", "rollout_large", "varlen_large", "group_large", "vit_large"]
SLACK_ROWS = 128                                                            # rows behind M_pad that every forward clears by hand


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def euler_walk(n):
    """A closed walk over vertices 0 .. n-1 that uses every ordered pair (i, j), i == j included, exactly once: n * n + 1 vertices
    (Hierholzer on the complete digraph with loops; deterministic)."""
    todo = [list(range(n)) for _ in range(n)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if todo[v]:
            stack.append(todo[v].pop(0))
        else:
            walk.append(stack.pop())
    return walk[::-1]


def plan():
    """Catalogue names: an Eulerian walk over the kinds (65 calls for 8 kinds), every kind alternating between its geometries from visit
    to visit, the small one first -- so the walk goes small -> large -> small for the workspace and for forward_rollout's own."""
    sizes = {k: [e.name for e in _ENTRIES if e.kind == k] for k in KINDS}
    seen = dict.fromkeys(KINDS, 0)
    names = []
    for v in euler_walk(len(KINDS)):
        k = KINDS[v]
        names.append(sizes[k][seen[k] % len(sizes[k])])
        seen[k] += 1
    return names


# ---- models and the fresh-engine reference ---------------------------------------------------------------------------------------------
_state = {}


def state_dict(wseed=WSEED, weights="plain"):
    """numpy weights of synth.make_state_dict; "gain1e7": the 1e7-gain attention_norm channels of test_default_model_has_no_silent_nans
    (fp16 operands overflow, bf16x3 stays finite)."""
    key = (wseed, weights)
    if key not in _state:
        sd = synth.make_state_dict(spec(), wseed)
        if weights == "gain1e7":
            sd["transformer.encoder.layers.0.attention_norm.weight"][:4] *= 1e7
        _state[key] = sd
    return _state[key]


def build_model(precision, options=0, token=0, wseed=WSEED, weights="plain"):
    m = VTAMIQ(**json.loads(json.dumps(KW)), precision=precision, engine_options=options)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict(wseed, weights).items()})
    m.token_num = token
    return m.to(DEV).eval()


def fresh_outputs(name, precision, options=0, token=0, wseed=WSEED, weights="plain", inp=None):
    """The call on a freshly constructed model -- a new engine that runs nothing else -- after a full synchronize, cloned."""
    torch.cuda.synchronize()
    m = build_model(precision, options, token, wseed, weights)
    out = CATALOGUE[name].run(m, inp)
    torch.cuda.synchronize()
    out = tuple(t.clone() for t in out)
    del m
    return out


_refs = {}


def reference(name, precision, options=0, token=0, wseed=WSEED, weights="plain"):
    """fresh_outputs of the catalogue entry's own inputs: computed once per configuration, shared by the tests, never modified."""
    key = (name, precision, options, token, wseed, weights)
    if key not in _refs:
        _refs[key] = fresh_outputs(name, precision, options, token, wseed, weights)
    return _refs[key]


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def compare(results, refs):
    """results: [(catalogue name, outputs)] in call order; refs: name -> reference outputs.  -> one line per output tensor that does not
    have the reference's bits, naming the call: "call 17 rollout_small output 1: ..." (empty: everything equal)."""
    lines = []
    for i, (name, outs) in enumerate(results):
        want = refs[name]
        if len(outs) != len(want):
            lines.append(f"call {i} {name}: {len(outs)} outputs, the fresh engine gives {len(want)}")
            continue
        for k, (a, b) in enumerate(zip(outs, want)):
            if not same_bits(a, b):
                n = int((bits(a) != bits(b)).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1
                lines.append(f"call {i} {name} output {k}: {n} of {a.numel()} elements differ from the fresh engine's")
    return lines


def compare_masked(outs, want):
    """Outputs of a call whose inputs held NaN against the same call's on another engine: the same NaN mask, the same bits elsewhere.
    -> lines as compare()."""
    lines = []
    for k, (a, b) in enumerate(zip(outs, want)):
        if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
            lines.append(f"output {k}: NaN mask differs")
        elif not torch.equal(bits(torch.nan_to_num(a, nan=0.0)), bits(torch.nan_to_num(b, nan=0.0))):
            lines.append(f"output {k}: bits differ outside the NaN mask")
    if len(outs) != len(want):
        lines.append(f"{len(outs)} outputs against {len(want)}")
    return lines


def all_pairs_differ(refs):
    """The first outputs of any two different entries differ (equality with a reference is no empty statement)."""
    for (a, x), (b, y) in itertools.combinations(refs.items(), 2):
        if x[0].shape == y[0].shape and torch.equal(x[0], y[0]):
            return f"{a} and {b} have the same first output"
    return None
