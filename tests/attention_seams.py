"""Inputs and fp64 references for the key-masking attention kernels at the seam lengths (no GPU code: importable anywhere).

Eight kernels decide by a sequence's length S which keys and query rows belong to it: the 4-wave, pipelined and split attention kernels,
attention_varlen_kernel, attention_probs_kernel and the rollout step / combine kernels in their uniform and table-driven forms.  On Gaussian
Q and K every key holds about 1/S of a row's probability, so a mask that is off by one key moves the answer by about 1/S^2: far below the
bounds of the single-plane formats.  The inputs made here put a third to a half of every row's probability on key S - 1 and the same weight
on every row a kernel may load but must mask, so an off-by-one mask is the largest term of the error
(tests/test_attention_seams.py proves that on the CPU; tests/test_gpu_attention_seams.py runs the kernels).

Construction, for packed sequences of given lengths (pitches: rows from one sequence's first row to the next one's; the length itself when
packed back to back):
    base      qkv = BASE * randn, one seeded draw shared by every case (base_rows)
    u_h       one unit vector per head, the same for every sequence
    Q         every row of a sequence of length S gets + (8 (ln S + MARGIN) / b) u_h, b = sqrt(8 (ln 513 + MARGIN)): q . k_spike / 8 is about
              ln S + MARGIN against ANY spike key, whichever sequence it belongs to
    K spikes  b u_h + 0.1 (base K) in row 0 and row S - 1 of every sequence, in its pad rows [S, pitch) and in the SLACK rows behind the last
              sequence (packed: the row behind S - 1 is the next sequence's row 0, which carries the spike already)
    V         base scale everywhere: an admitted key moves the output as well
A spike key weighs S e^MARGIN, about 4 times all ordinary keys of its row together, so key S - 1 holds 0.25 .. 0.55 of each row (the most at
S = 2 and 3, where the spikes are nearly all the keys); logits stay below 9.5.  MARGIN and BASE are set by the CPU condition alone.

References take the VALUES the operand planes hold (planes_value) as one fp64 (rows, 3H) tensor and work per sequence.  Each has three
deliberately wrong variants: "drop_last" (keys [0, S - 1)), "admit_next" (keys [0, S], taking row S of the buffer) and "count_last_twice"
(key S - 1 twice: what the clamped loads of the probs and rollout kernels would give if the clamped copy were not masked)."""
import functools
import math

import torch

SEAMS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 385, 511, 512, 513]
GRANULES = (32, 64, 128, 256)          # rows of a wave, keys of a tile, the query block of the 4-wave / probs / rollout kernels, of the pipelined one
SLACK = 128                            # rows behind the last sequence (vtq_k_attention reads up to 127 of them)
HEAD_DIM = 64
BASE = 0.5
MARGIN = 1.5
SPIKE = math.sqrt(8.0 * (math.log(513.0) + MARGIN))       # b, about 7.87
WRONG = ("drop_last", "admit_next", "count_last_twice")
Q_LOG2_SCALE = 0.125 * math.log2(math.e)                  # what the 3-term formats' query projection folds into Q


def starts_of(lengths, pitches=None):
    """First row of every sequence, and the rows all of them span."""
    pitches = list(lengths) if pitches is None else list(pitches)
    assert len(pitches) == len(lengths) and all(p >= s >= 1 for s, p in zip(lengths, pitches))
    starts, row = [], 0
    for p in pitches:
        starts.append(row)
        row += p
    return starts, row


@functools.lru_cache(maxsize=None)
def base_rows(nh=12, rows=sum(SEAMS) + SLACK, seed=1607):
    """The one seeded draw: (rows, 3 nh 64) fp32 at BASE scale and the (nh, 64) unit vectors.  Never modified (make_qkv copies)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.randn(nh, HEAD_DIM, generator=g, dtype=torch.float64)
    u = (u / u.norm(dim=-1, keepdim=True)).float()
    return BASE * torch.randn(rows, 3 * nh * HEAD_DIM, generator=g), u


def make_qkv(lengths, pitches=None, base=None, u=None):
    """fp32 (rows + SLACK, 3H) on base's device; base, u as base_rows() gives them (or copies of them on another device)."""
    if base is None:
        base, u = base_rows()
    nh = u.shape[0]
    H = nh * HEAD_DIM
    starts, rows = starts_of(lengths, pitches)
    pitches = list(lengths) if pitches is None else list(pitches)
    assert rows + SLACK <= base.shape[0] and base.shape[1] == 3 * H
    qkv = base[:rows + SLACK].clone()
    spike = torch.zeros(rows + SLACK, dtype=torch.bool, device=base.device)
    spike[rows:] = True
    uf = u.reshape(1, H).to(base.device)
    for r0, S, pitch in zip(starts, lengths, pitches):
        qkv[r0:r0 + pitch, :H] += (8.0 * (math.log(S) + MARGIN) / SPIKE) * uf
        spike[r0] = True
        spike[r0 + S - 1:r0 + pitch] = True
    k = qkv[:, H:2 * H]
    k[spike] = SPIKE * uf + 0.1 * k[spike]
    return qkv


def rollout_inputs(S, seed=0):
    """The three r_in of a sequence, fp32 (3, S): random positive summing to 1, one-hot at row S - 1 (the result is then
    1/2 e + 1/2 mean_h P[S - 1, :]: the last query row alone), one-hot at row 0."""
    g = torch.Generator(device="cpu").manual_seed(4242 + 7 * S + seed)
    r = torch.zeros(3, S, dtype=torch.float64)
    r[0] = torch.rand(S, generator=g, dtype=torch.float64) + 0.05
    r[0] /= r[0].sum()
    r[1, S - 1] = 1.0
    r[2, 0] = 1.0
    return r.float()


R_KINDS = ("random", "one-hot S-1", "one-hot 0")


# ---- fp64 references -------------------------------------------------------------------------------------------------------------------------
def key_rows(r0, S, variant="true"):
    rows = {"true": list(range(r0, r0 + S)), "drop_last": list(range(r0, r0 + S - 1)), "admit_next": list(range(r0, r0 + S + 1)),
            "count_last_twice": list(range(r0, r0 + S)) + [r0 + S - 1]}[variant]
    return rows


def _probs_over(val, r0, S, variant, nq, q_scale):
    """softmax over the variant's key list: ((nh, nq, keys) fp64, the key rows).  No key at all (drop_last at S = 1): NaN."""
    H = val.shape[1] // 3
    nh = H // HEAD_DIM
    idx = torch.tensor(key_rows(r0, S, variant), dtype=torch.long, device=val.device)
    q = val[r0:r0 + nq, :H].double().view(nq, nh, HEAD_DIM).permute(1, 0, 2) / q_scale
    k = val[idx, H:2 * H].double().view(len(idx), nh, HEAD_DIM).permute(1, 0, 2)
    if len(idx) == 0:
        return torch.full((nh, nq, 0), float("nan"), dtype=torch.float64, device=val.device), idx
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1), idx


def probs_ref(val, r0, S, variant="true", nq=None, q_scale=1.0):
    """(nh, nq, S): what a kernel with this mask would store for the keys [0, S) of the sequence at row r0 (nq query rows, default S)."""
    nq = S if nq is None else nq
    p, idx = _probs_over(val, r0, S, variant, nq, q_scale)
    out = torch.zeros(p.shape[0], nq, S, dtype=torch.float64, device=val.device)
    if len(idx) == 0:
        return out + float("nan")
    n = min(len(idx), S)
    out[:, :, :n] = p[:, :, :n]
    return out


def attention_ref(val, r0, S, variant="true", nq=None, q_scale=1.0):
    """(nq, H): softmax(Q K^T / 8) V over the variant's keys, heads merged."""
    nq = S if nq is None else nq
    H = val.shape[1] // 3
    p, idx = _probs_over(val, r0, S, variant, nq, q_scale)
    if len(idx) == 0:
        return torch.full((nq, H), float("nan"), dtype=torch.float64, device=val.device)
    v = val[idx, 2 * H:].double().view(len(idx), p.shape[0], HEAD_DIM).permute(1, 0, 2)
    return (p @ v).permute(1, 0, 2).reshape(nq, H)


def rollout_ref(r, P):
    """1/2 r + 1/2 mean_h r^T P for r (.., S) and P (nh, S, S) as probs_ref gives it."""
    r = r.double()
    return 0.5 * r + 0.5 * torch.einsum("...i,hij->...j", r, P) / P.shape[0]


def row_distance(a, b):
    """max |a - b| over the last dimension; a NaN on either side is an infinite distance."""
    d = (a - b).abs()
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).amax(-1)
