"""One-to-many scoring on images of different patch counts against what a user did before it (profiles/r12_group_varlen.txt).

    python tools/group_varlen_bench.py [--out profiles/r12_group_varlen.txt] [--steps 20] [--warmup 5] [--reps 5] [--parent-lib PATH]

ViT-B/16, L = 12, precision fp16x3 (explicit: no error-word read per call).  G = 4 references of 300 / 400 / 500 / 600 patches, 8 distorted
images each with their reference's count (M = 32), inputs resident on the device.  HIP events around `steps` back-to-back calls after
`warmup` calls, `reps` repetitions with the variants interleaved inside each repetition:
    (a) group_varlen      forward_group(lengths=...) on the 4 + 32 = 36 sequences
    (b) varlen_expanded   forward_varlen on the 32 expanded pairs: 64 sequences, every reference encoded 8 times
    (c) group_per_size    four uniform forward_group calls, one per size (1 + 8 sequences each)
    (d) encode + cached   encode_reference(lengths=...) + forward_cached(lengths=...) per call; the cached call alone as well
    (v) varlen_same       forward_varlen at the SAME sequence and row count: 18 pairs, 5 / 4 / 4 / 5 of 300 / 400 / 500 / 600 patches
--parent-lib: a build of the parent commit's csrc/ (python -m vtamiq_amd.build in a checkout of it).  (b) and (c) then run on THAT library
as well, on an engine of their own in the same process and the same interleaved repetitions -- the comparison the README row quotes.  The
parent library lacks this commit's entries: it loads with VTQ_ALLOW_ABI_MISMATCH=1 (vtamiq_amd/_lib.py).
No ratio is a bar here: the expectations -- (a) close to (v), (a) below (b) by roughly the share of sequences saved, 36 / 64 -- are printed
beside what was measured."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, _lib, synth  # noqa: E402

DEV = "cuda"
SIZES, PER_REF = [300, 400, 500, 600], 8
bits = lambda t: t.contiguous().view(torch.int32)


class ParentVTAMIQ(VTAMIQ):
    """The same model on another build of the engine library."""
    LIB = None

    def _engine_lib(self):
        return _lib.load(self.LIB)


def make_model(cls=VTAMIQ):
    m = cls(vit_config=dict(variant="ViT-B16", pretrained=False), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 0).items()})
    return m.to(DEV).eval()


def images(spec, counts, seed, dist):
    """Per-image device tensors [(patches (n, 3, P, P), pos (n, 2))]."""
    out = []
    for i, n in enumerate(counts):
        pa, po, _ = synth.make_inputs(spec, 1, n, seed + i, aligned=False)
        out.append((torch.from_numpy(pa[0, int(dist)]).to(DEV), torch.from_numpy(po[0, int(dist)]).to(DEV)))
    return out


def timed(fn, steps, warmup):
    """ms per call: HIP events around `steps` calls behind `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r12_group_varlen.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/group_varlen_bench.py measures on the GPU: no device found")
    if a.steps < 20 or a.warmup < 5 or a.reps < 5:
        print("[group_varlen_bench] fewer than 20 steps / 5 warm-ups / 5 repetitions: not the protocol of profiles/r12_group_varlen.txt", file=sys.stderr)
    model = make_model()
    spec = model.spec
    G, M = len(SIZES), len(SIZES) * PER_REF
    index = [m // PER_REF for m in range(M)]                       # distorted images grouped by reference
    n_ref, n_dist = list(SIZES), [SIZES[i] for i in index]
    refs, dists = images(spec, n_ref, 11, False), images(spec, n_dist, 100, True)
    cat = lambda imgs, k: torch.cat([im[k] for im in imgs])
    pr, qr, pd, qd = cat(refs, 0), cat(refs, 1), cat(dists, 0), cat(dists, 1)
    # (b): every pair with its own copy of the reference
    er = [refs[i] for i in index]
    epr, eqr = cat(er, 0), cat(er, 1)
    # (c): per size one uniform group of 1 reference and its 8 distorted images
    per_size = []
    for g in range(G):
        ds = dists[g * PER_REF:(g + 1) * PER_REF]
        per_size.append(((refs[g][0][None], torch.stack([d[0] for d in ds])), (refs[g][1][None], torch.stack([d[1] for d in ds]))))
    # (v): 18 pairs = 36 sequences with the same number of token rows: (a) holds 9 sequences of each size, pairs come in twos, so 5 / 4 / 4 / 5
    # pairs of 300 / 400 / 500 / 600 patches (10 + 8 + 8 + 10 sequences, 16200 patches as in (a)); timing only, images may repeat
    left, right = [], []
    for g, k in enumerate((5, 4, 4, 5)):
        left += [dists[g * PER_REF + j] for j in range(k)]
        right += [dists[g * PER_REF + (j + 3) % PER_REF] for j in range(k)]
    n_same = [x[0].shape[0] for x in left]
    assert len(n_same) == (G + M) // 2 and 2 * sum(n_same) == sum(n_ref) + sum(n_dist)
    spl, sql, spr, sqr = cat(left, 0), cat(left, 1), cat(right, 0), cat(right, 1)

    def variants_of(m, only=None):
        v = {
            "group_varlen": lambda: m.forward_group((pr, pd), (qr, qd), (None, None), index, lengths=(n_ref, n_dist))[0],
            "varlen_expanded": lambda: m.forward_varlen((epr, pd), (eqr, qd), (None, None), n_dist)[0],
            "group_per_size": lambda: torch.cat([m.forward_group(p, q, (None, None), [0] * PER_REF)[0] for p, q in per_size]),
            "encode+cached": lambda: m.forward_cached(m.encode_reference(pr, qr, lengths=n_ref), pd, qd, None, index, lengths=n_dist)[0],
            "varlen_same": lambda: m.forward_varlen((spl, spr), (sql, sqr), (None, None), n_same)[0],
        }
        return {k: f for k, f in v.items() if only is None or k in only}

    with torch.no_grad():
        variants = variants_of(model)
        ref = model.encode_reference(pr, qr, lengths=n_ref)
        variants["cached_alone"] = lambda: model.forward_cached(ref, pd, qd, None, index, lengths=n_dist)[0]
        if a.parent_lib:
            ParentVTAMIQ.LIB = a.parent_lib
            parent = make_model(ParentVTAMIQ)
            for k, f in variants_of(parent, ("varlen_expanded", "group_per_size")).items():
                variants[k + " [parent]"] = f
        # the scoring forms agree bit for bit before anything is timed (counts are equal pairwise: the single pair's bits everywhere)
        scoring = [k for k in variants if k != "varlen_same"]
        q = {k: variants[k]() for k in scoring}
        torch.cuda.synchronize()
        same = all(torch.equal(bits(q["group_varlen"]), bits(x)) for x in q.values()) and bool(torch.isfinite(q["group_varlen"]).all())
        assert same, "the scoring forms disagree"
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.steps, a.warmup))
    st = {k: stats(v) for k, v in times.items()}
    nseq = {"group_varlen": G + M, "varlen_expanded": 2 * M, "group_per_size": G + M, "encode+cached": G + M, "varlen_same": G + M, "cached_alone": M}
    lines = [f"tools/group_varlen_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit); G = {G} references of "
             f"{' / '.join(map(str, SIZES))} patches, {PER_REF} distorted images each (M = {M})",
             f"ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved; "
             f"[parent] = the parent commit's library ({'given' if a.parent_lib else 'NOT given: this library only'})", "",
             f"{'variant':<28}{'sequences':>10}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
    for k, s in st.items():
        lines.append(f"{k:<28}{nseq[k.split(' [')[0]]:>10}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{t:.3f}" for t in times[k]))
    med = {k: s["median"] for k, s in st.items()}
    b = med.get("varlen_expanded [parent]", med["varlen_expanded"])
    c = med.get("group_per_size [parent]", med["group_per_size"])
    base = "the parent's library" if a.parent_lib else "this library"
    lines += ["",
              f"(a) / (b) = group_varlen / varlen_expanded on {base} = {med['group_varlen'] / b:.3f}   (expectation: roughly the share of sequences, "
              f"{(G + M) / (2 * M):.3f})",
              f"(a) / (c) = group_varlen / group_per_size on {base} = {med['group_varlen'] / c:.3f}",
              f"(a) / (v) = group_varlen / varlen_same = {med['group_varlen'] / med['varlen_same']:.3f}   (expectation: close to 1, the same kernels at "
              f"the same {G + M} sequences)",
              f"(d) / (b) = (encode + cached) / varlen_expanded = {med['encode+cached'] / b:.3f};   cached alone / (b) = {med['cached_alone'] / b:.3f}"]
    if a.parent_lib:
        lines.append(f"this library / the parent's on the unchanged calls: varlen_expanded {med['varlen_expanded'] / med['varlen_expanded [parent]']:.3f}, "
                     f"group_per_size {med['group_per_size'] / med['group_per_size [parent]']:.3f}")
    lines += ["scores bit-identical across every scoring form (this library and the parent's): True", "",
              "json: " + json.dumps(dict(times=st, sequences=nseq))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
