#!/usr/bin/env python3
"""forward_varlen against what a user did before it (GPU box; profiles/r09_varlen.txt): ViT-B/16, 12 layers, precision fp16x3.

  (a) 32 pairs of mixed patch counts over {200, 350, 500, 650, 800} (sum = 32 x 500) through ONE forward_varlen call
  (b) the same pairs grouped by patch count into uniform forward() calls, one per distinct count
  (c) forward() at B = 32, N = 500                      (d) forward_varlen with 32 x 500
  (e) eight single-pair requests of different N: one forward_varlen call against eight forward() calls

Every ratio comes from this one run: each variant is warmed up at its own shapes, then the variants are timed alternately in rounds (HIP
events around a window of `--iters` calls each; the median round is quoted, the spread beside it).  Scores are compared bit for bit where
the contract says they are equal."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vtamiq_amd import VTAMIQ, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--precision", default="fp16x3")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("varlen_bench: no GPU (timings are taken on the MI355X only)")
dev = torch.device("cuda")
m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=args.layers, pretrained=False), precision=args.precision)
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 0).items()})
m = m.to(dev).eval()

# 32 lengths over the five counts, summing to 32 x 500 (6 x 200, 7 x 350, 6 x 500, 7 x 650, 6 x 800), in a fixed shuffled order
MIXED = [500, 200, 800, 350, 650, 350, 650, 200, 500, 800, 650, 350, 200, 800, 500, 650, 350, 200, 800, 500, 650, 350, 500, 200, 800, 650,
         350, 500, 200, 800, 350, 650]
assert len(MIXED) == 32 and sum(MIXED) == 32 * 500
SINGLES = [50, 120, 200, 350, 500, 650, 800, 1024]


def inputs(lengths, seed):
    """per-pair device tensors [(patches_ref, patches_dist, pos_ref, pos_dist)] of lengths[b] patches"""
    out = []
    for b, n in enumerate(lengths):
        pa, po, _ = synth.make_inputs(m.spec, 1, n, seed + b, aligned=False)
        out.append(tuple(torch.from_numpy(a[0, i]).to(dev) for a in (pa, po) for i in (0, 1)))
    return out


def varlen_call(pairs, lengths):
    cat = lambda i: torch.cat([p[i] for p in pairs])
    pr, pd, qr, qd = cat(0), cat(1), cat(2), cat(3)
    return lambda: m.forward_varlen((pr, pd), (qr, qd), (None, None), lengths)[0]


def grouped_call(pairs, lengths):
    """one uniform forward() per distinct length; returns the scores in the pairs' order"""
    groups = {}
    for b, n in enumerate(lengths):
        groups.setdefault(n, []).append(b)
    batches = []
    for n, idx in sorted(groups.items()):
        st = lambda i: torch.stack([pairs[b][i] for b in idx])
        batches.append((idx, st(0), st(1), st(2), st(3)))
    order = torch.tensor([b for idx, *_ in batches for b in idx], device=dev)

    def call():
        q = torch.cat([m((pr, pd), (qr, qd), (None, None))[0] for _, pr, pd, qr, qd in batches])
        out = torch.empty_like(q)
        out[order] = q
        return out
    return call, len(batches)


def time_all(calls):
    """{name: call} -> {name: [ms per call, one per round]}: warm-up of every variant, then alternating timed windows"""
    for c in calls.values():
        for _ in range(3):
            c()
    torch.cuda.synchronize()
    res = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, c in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                c()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / args.iters)
    return res


fmt = lambda v: f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
bits = lambda t: t.contiguous().view(torch.int32)
with torch.no_grad():
    mixed = inputs(MIXED, 100)
    uni = inputs([500] * 32, 200)
    singles = inputs(SINGLES, 300)
    a = varlen_call(mixed, MIXED)
    b, nb = grouped_call(mixed, MIXED)
    c, _ = grouped_call(uni, [500] * 32)
    d = varlen_call(uni, [500] * 32)
    e1 = varlen_call(singles, SINGLES)
    e8, _ = grouped_call(singles, SINGLES)
    same = {"a == b": torch.equal(bits(a()), bits(b())), "d == c": torch.equal(bits(d()), bits(c())), "e: one call == eight calls": torch.equal(bits(e1()), bits(e8()))}
    t = time_all({"a": a, "b": b, "c": c, "d": d, "e1": e1, "e8": e8})
med = {k: statistics.median(v) for k, v in t.items()}
print(f"varlen_bench: ViT-B/16, {args.layers} layers, precision {args.precision}, {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.iters} calls, "
      "HIP events; median round (min, max)")
print(f"(a) forward_varlen, 32 pairs, N over {{200, 350, 500, 650, 800}}, sum 16000      {fmt(t['a'])}")
print(f"(b) the same pairs as {nb} uniform forward() calls, one per patch count          {fmt(t['b'])}")
print(f"(c) forward(), B = 32, N = 500                                               {fmt(t['c'])}")
print(f"(d) forward_varlen, 32 x 500                                                 {fmt(t['d'])}")
print(f"(e) 8 single pairs, N = {SINGLES}: one forward_varlen call   {fmt(t['e1'])}")
print(f"    the same as eight forward() calls                                        {fmt(t['e8'])}")
print(f"a / b = {med['a'] / med['b']:.3f}    d / c = {med['d'] / med['c']:.3f}    e (one call / eight calls) = {med['e1'] / med['e8']:.3f}")
print("scores bit-identical: " + ", ".join(f"{k}: {v}" for k, v in same.items()))
