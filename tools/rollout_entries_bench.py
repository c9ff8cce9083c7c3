"""Attention rollout through the variable-length, group and cached entries against what a user did before them
(profiles/r14_rollout_entries.txt).

    python tools/rollout_entries_bench.py [--out profiles/r14_rollout_entries.txt] [--steps 20] [--warmup 5] [--reps 5] [--parent-lib PATH]

ViT-B/16, L = 12, precision fp16x3 (explicit: no error-word read per call), inputs resident on the device.  HIP events around `steps`
back-to-back calls after `warmup` calls, `reps` repetitions with every variant interleaved inside each repetition, all in one process:
    (a) 32 pairs of 300 / 400 / 500 / 600 patches (8 of each)
        a_ragged_rollout     forward_rollout(lengths=...)                           64 sequences, one call
        a_single_rollouts    32 forward_rollout calls, one pair each                64 sequences, 32 calls -- the maps before this change
        a_varlen             forward_varlen on the same batch                       the scores alone
    (b) G = 4 references, M = 32 distorted images (8 each), N = 500
        b_group_rollout      forward_group(rollout=True)                            36 sequences
        b_expanded_rollout   forward_rollout on the 32 expanded pairs               64 sequences, every reference encoded 8 times
        b_group              forward_group                                          the scores alone
    (c) the lengths= group of profiles/r12_group_varlen.txt: 4 references of 300 / 400 / 500 / 600 patches, 8 distorted images each
        c_group_rollout      forward_group(lengths=..., rollout=True)               36 sequences
        c_expanded_rollout   forward_rollout(lengths=...) on the 32 expanded pairs  64 sequences
        c_group              forward_group(lengths=...)                             the scores alone
    (p) forward and forward_rollout at B = 32, N = 500: the entries this change does not alter.  With --parent-lib (a build of the parent
        commit's csrc/) they also run on THAT library, on an engine of its own, in the same repetitions.  The parent library lacks this
        commit's entries: it loads with VTQ_ALLOW_ABI_MISMATCH=1 (vtamiq_amd/_lib.py).
No ratio is a bar here.  What is known beforehand -- the uniform rollout costs 1.27 x forward (profiles/r11_rollout.txt), the group forms
0.59 - 0.61 x the expanded pairs (r10_group.txt, r12_group_varlen.txt), the share of sequences is 36 / 64 -- is printed beside what was measured."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, _lib, synth  # noqa: E402

DEV = "cuda"
SIZES, PER_REF, N_UNIFORM = [300, 400, 500, 600], 8, 500
bits = lambda t: t.contiguous().view(torch.int32)
same = lambda x, y: x.shape == y.shape and bool(torch.equal(bits(x), bits(y)))


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_rollout_entries.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/rollout_entries_bench.py measures on the GPU: no device found")
    if a.steps < 20 or a.warmup < 5 or a.reps < 5:
        print("[rollout_entries_bench] fewer than 20 steps / 5 warm-ups / 5 repetitions: not the protocol of profiles/r14_rollout_entries.txt", file=sys.stderr)
    model = make_model()
    spec = model.spec
    G, M = len(SIZES), len(SIZES) * PER_REF
    index = [m // PER_REF for m in range(M)]                       # distorted images grouped by reference
    cat = lambda imgs, k: torch.cat([im[k] for im in imgs])
    stack = lambda imgs, k: torch.stack([im[k] for im in imgs])
    none2 = (None, None)
    # (a) / (c): ragged images.  (a) pairs distorted image m with its own reference copy; (c) holds each reference once
    n_ref, n_dist = list(SIZES), [SIZES[i] for i in index]
    refs, dists = images(spec, n_ref, 11, False), images(spec, n_dist, 100, True)
    exp = [refs[i] for i in index]
    pr, qr, pd, qd, epr, eqr = cat(refs, 0), cat(refs, 1), cat(dists, 0), cat(dists, 1), cat(exp, 0), cat(exp, 1)
    single = [((exp[m][0][None], dists[m][0][None]), (exp[m][1][None], dists[m][1][None])) for m in range(M)]
    # (b) / (p): uniform images
    urefs, udists = images(spec, [N_UNIFORM] * G, 300, False), images(spec, [N_UNIFORM] * M, 400, True)
    uexp = [urefs[i] for i in index]
    upr, uqr, upd, uqd, uepr, ueqr = stack(urefs, 0), stack(urefs, 1), stack(udists, 0), stack(udists, 1), stack(uexp, 0), stack(uexp, 1)

    def unchanged(m):
        return {"forward": lambda: m((uepr, upd), (ueqr, uqd), none2)[0],
                "forward_rollout": lambda: m.forward_rollout((uepr, upd), (ueqr, uqd), none2)}

    with torch.no_grad():
        variants = {
            "a_ragged_rollout": lambda: model.forward_rollout((epr, pd), (eqr, qd), none2, lengths=n_dist),
            "a_single_rollouts": lambda: [model.forward_rollout(p, q, none2) for p, q in single],
            "a_varlen": lambda: model.forward_varlen((epr, pd), (eqr, qd), none2, n_dist)[0],
            "b_group_rollout": lambda: model.forward_group((upr, upd), (uqr, uqd), none2, index, rollout=True),
            "b_expanded_rollout": lambda: model.forward_rollout((uepr, upd), (ueqr, uqd), none2),
            "b_group": lambda: model.forward_group((upr, upd), (uqr, uqd), none2, index)[0],
            "c_group_rollout": lambda: model.forward_group((pr, pd), (qr, qd), none2, index, lengths=(n_ref, n_dist), rollout=True),
            "c_expanded_rollout": lambda: model.forward_rollout((epr, pd), (eqr, qd), none2, lengths=n_dist),
            "c_group": lambda: model.forward_group((pr, pd), (qr, qd), none2, index, lengths=(n_ref, n_dist))[0],
        }
        variants.update({"p_" + k: f for k, f in unchanged(model).items()})
        if a.parent_lib:
            ParentVTAMIQ.LIB = a.parent_lib
            parent = make_model(ParentVTAMIQ)
            variants.update({"p_" + k + " [parent]": f for k, f in unchanged(parent).items()})

        # ---- every form agrees bit for bit before anything is timed ------------------------------------------------------------------------
        qa, ra = variants["a_ragged_rollout"]()
        singles = variants["a_single_rollouts"]()
        ok = same(qa, variants["a_varlen"]())
        for m, (q1, r1) in enumerate(singles):
            ok = ok and same(qa[m:m + 1], q1) and all(same(ra.rollout[k][m], r1.rollout[k, 0]) and same(ra.last_attention[k][m], r1.last_attention[k, 0])
                                                      for k in (0, 1))
        qb, rb = variants["b_group_rollout"]()
        qe, re_ = variants["b_expanded_rollout"]()
        ok = ok and same(qb, qe) and same(qb, variants["b_group"]()) and same(rb.rollout[1], re_.rollout[1]) and same(rb.last_attention[1], re_.last_attention[1])
        ok = ok and all(same(rb.rollout[0][index[m]], re_.rollout[0, m]) for m in range(M))
        qc, rc = variants["c_group_rollout"]()
        ok = ok and same(qc, qa) and same(qc, variants["c_group"]())
        ok = ok and all(same(rc.rollout[1][m], ra.rollout[1][m]) and same(rc.rollout[0][index[m]], ra.rollout[0][m]) for m in range(M))
        if a.parent_lib:
            qp, rp = variants["p_forward_rollout [parent]"]()
            ok = ok and same(qp, qe) and same(rp.rollout, re_.rollout) and same(rp.last_attention, re_.last_attention)
            ok = ok and same(variants["p_forward [parent]"](), variants["p_forward"]())
        torch.cuda.synchronize()
        assert ok and bool(torch.isfinite(qa).all()) and bool(torch.isfinite(qb).all()), "the forms disagree"

        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.steps, a.warmup))
    st = {k: stats(v) for k, v in times.items()}
    nseq = {"a_ragged_rollout": 2 * M, "a_single_rollouts": 2 * M, "a_varlen": 2 * M, "b_group_rollout": G + M, "b_expanded_rollout": 2 * M, "b_group": G + M,
            "c_group_rollout": G + M, "c_expanded_rollout": 2 * M, "c_group": G + M, "p_forward": 2 * M, "p_forward_rollout": 2 * M}
    lines = [f"tools/rollout_entries_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit); (a) {M} pairs of "
             f"{' / '.join(map(str, SIZES))} patches; (b) G = {G}, M = {M}, N = {N_UNIFORM}; (c) {G} references of {' / '.join(map(str, SIZES))} patches, "
             f"{PER_REF} distorted images each; (p) B = {M}, N = {N_UNIFORM}",
             f"ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved in one process; "
             f"[parent] = the parent commit's library ({'given' if a.parent_lib else 'NOT given: this library only'})", "",
             f"{'variant':<34}{'sequences':>10}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions"]
    for k, s in st.items():
        lines.append(f"{k:<34}{nseq[k.split(' [')[0]]:>10}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{t:.3f}" for t in times[k]))
    med = {k: s["median"] for k, s in st.items()}
    share = (G + M) / (2 * M)
    lines += ["",
              f"(a) ragged rollout / 32 single-pair rollouts = {med['a_ragged_rollout'] / med['a_single_rollouts']:.3f}   (the same 64 sequences: what one call saves over 32)",
              f"(a) ragged rollout / forward_varlen          = {med['a_ragged_rollout'] / med['a_varlen']:.3f}   (known for the uniform entry: 1.27 x forward; measured "
              f"here: {med['p_forward_rollout'] / med['p_forward']:.3f})",
              f"(b) group rollout / expanded-pair rollout    = {med['b_group_rollout'] / med['b_expanded_rollout']:.3f}   (share of sequences {share:.3f}; known for the scores: 0.59)",
              f"(b) group rollout / forward_group            = {med['b_group_rollout'] / med['b_group']:.3f}",
              f"(c) group rollout / expanded-pair rollout    = {med['c_group_rollout'] / med['c_expanded_rollout']:.3f}   (share of sequences {share:.3f}; known for the scores: 0.61)",
              f"(c) group rollout / forward_group(lengths)   = {med['c_group_rollout'] / med['c_group']:.3f}"]
    if a.parent_lib:
        lines.append(f"(p) this library / the parent's on the unchanged entries: forward {med['p_forward'] / med['p_forward [parent]']:.3f}, "
                     f"forward_rollout {med['p_forward_rollout'] / med['p_forward_rollout [parent]']:.3f}")
    lines += ["scores and maps bit-identical across the forms of each case" + (", forward / forward_rollout across the two libraries" if a.parent_lib else "") + ": True",
              "", "json: " + json.dumps(dict(times=st, sequences=nseq))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
