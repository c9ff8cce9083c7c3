"""One-to-many scoring against forward(): what encoding every reference once buys (profiles/r10_group.txt).

    python tools/group_bench.py [--out profiles/r10_group.txt] [--steps 20] [--warmup 5] [--reps 5]

ViT-B/16, L = 12, N = 500 patches, precision fp16x3 (explicit: no error-word read per call).  For G references and M = 32 distorted images
(G = 4 and G = 1) it times, with HIP events around `steps` back-to-back calls after `warmup` calls, `reps` repetitions with the variants
interleaved inside each repetition:
    group      forward_group on G + M sequences
    cached     forward_cached on M sequences (the references encoded once, outside the timed loop; that one encode_reference is timed alone)
    expanded   forward on the 32 expanded pairs: 2 M sequences
    fwd_same   the unchanged forward at the SAME sequence count: B = (G + M) / 2 for the group (G = 4: B = 18), B = M / 2 = 16 for the cached form
The bar is not a fixed ratio: group / cached may exceed fwd_same's median by no more than fwd_same's own min-to-max spread over the repetitions
plus the measured time of the head's extra rows (head batch M against B; the "head" kernel class of profile_enable, which also holds the
CLS tail -- the same in both, the sequence counts being equal).  A missed bar is reported with the per-class profile, never moved."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, _lib, synth  # noqa: E402

DEV = "cuda"
N, M = 500, 32


def make_model():
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", pretrained=False), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 0).items()})
    return m.to(DEV).eval()


def images(spec, count, seed):
    pa, po, _ = synth.make_inputs(spec, count, N, seed, aligned=False)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(pa[:, 0]), t(pa[:, 1]), t(po[:, 0]), t(po[:, 1])


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


def per_class(model, fn, steps):
    """ms per call of every kernel class (HIP events around each launch: a run of its own, slower than the bare steps)."""
    model.profile_enable(_lib.KERNEL_CLASSES)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    prof = model.profile_collect()
    model.profile_enable([])
    return {k: ms / steps for k, (ms, _) in prof.items()}


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))


def measure(model, G, a, lines, record):
    spec = model.spec
    pr, _, qr, _ = images(spec, G, 11)
    _, pd, _, qd = images(spec, M, 12)
    index = [m % G for m in range(M)]
    idx = torch.tensor(index, device=DEV)
    exp = ((pr[idx].contiguous(), pd), (qr[idx].contiguous(), qd), (None, None))
    B_same, B_half = (G + M + 1) // 2, M // 2
    sp, sd, sq, sqd = images(spec, B_same, 13)
    same = ((sp, sd), (sq, sqd), (None, None))
    half = ((sp[:B_half].contiguous(), sd[:B_half].contiguous()), (sq[:B_half].contiguous(), sqd[:B_half].contiguous()), (None, None))
    with torch.no_grad():
        ref = model.encode_reference(pr, qr)
        variants = {
            "group": lambda: model.forward_group((pr, pd), (qr, qd), (None, None), index),
            "cached": lambda: model.forward_cached(ref, pd, qd, None, index),
            "expanded": lambda: model(*exp),
            f"fwd_same(B={B_same})": lambda: model(*same),
            f"fwd_half(B={B_half})": lambda: model(*half),
            "encode_reference": lambda: model.encode_reference(pr, qr),
        }
        # the three scoring forms agree bit for bit before anything is timed
        q = [variants[k]()[0] for k in ("group", "cached", "expanded")]
        torch.cuda.synchronize()
        assert all(torch.equal(q[0].view(torch.int32), x.view(torch.int32)) for x in q[1:]) and bool(torch.isfinite(q[0]).all())
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.steps, a.warmup))
        prof = {k: per_class(model, variants[k], a.steps) for k in ("group", "cached", f"fwd_same(B={B_same})", f"fwd_half(B={B_half})")}
    st = {k: stats(v) for k, v in times.items()}
    lines.append(f"== G = {G}, M = {M}, N = {N}: ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events), variants interleaved")
    lines.append(f"{'variant':<22}{'sequences':>10}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions")
    nseq = {"group": G + M, "cached": M, "expanded": 2 * M, f"fwd_same(B={B_same})": 2 * B_same, f"fwd_half(B={B_half})": 2 * B_half, "encode_reference": G}
    for k, s in st.items():
        lines.append(f"{k:<22}{nseq[k]:>10}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{t:.3f}" for t in times[k]))
    e = st["expanded"]["median"]
    lines.append(f"group / expanded = {st['group']['median'] / e:.3f} (sequence count predicts {(G + M) / (2 * M):.3f});   "
                 f"cached / expanded = {st['cached']['median'] / e:.3f} (predicts 0.500);   "
                 f"(encode_reference once + cached) / expanded = {(st['encode_reference']['median'] + st['cached']['median']) / e:.3f}")
    bars = {}
    for form, base in (("group", f"fwd_same(B={B_same})"), ("cached", f"fwd_half(B={B_half})")):
        head_extra = prof[form]["head"] - prof[base]["head"]
        margin = st[base]["spread"] + max(head_extra, 0.0)
        excess = st[form]["median"] - st[base]["median"]
        ok = excess <= margin
        rows = M - int(base.split("=")[1].rstrip(")"))
        lines.append(f"bar {form} vs {base}: excess {excess:+.3f} ms; allowed {margin:.3f} ms = spread of {base} {st[base]['spread']:.3f} + head time of the "
                     f"{rows} extra rows {head_extra:+.3f} (head class {prof[form]['head']:.3f} vs {prof[base]['head']:.3f}): {'MET' if ok else 'MISSED'}")
        bars[form] = dict(excess_ms=excess, margin_ms=margin, head_extra_ms=head_extra, met=ok)
    lines.append("per-class ms per call (events around every launch, a run of its own):")
    lines.append(f"{'':<22}" + "".join(f"{c:>12}" for c in _lib.KERNEL_CLASSES))
    for k, p in prof.items():
        lines.append(f"{k:<22}" + "".join(f"{p[c]:>12.3f}" for c in _lib.KERNEL_CLASSES))
    lines.append("")
    record[f"G{G}"] = dict(times=st, bars=bars, profile=prof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_group.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/group_bench.py measures on the GPU: no device found")
    if a.steps < 20 or a.warmup < 5 or a.reps < 5:
        print("[group_bench] fewer than 20 steps / 5 warm-ups / 5 repetitions: not the protocol of profiles/r10_group.txt", file=sys.stderr)
    model = make_model()
    lines = [f"tools/group_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, N = {N}, precision fp16x3 (explicit), M = {M} distorted images", ""]
    record = {}
    for G in (4, 1):
        measure(model, G, a, lines, record)
    lines.append("json: " + json.dumps(record))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
