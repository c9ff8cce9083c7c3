"""forward_rollout against forward() and against the route a user had before it (profiles/r11_rollout.txt).

    python tools/rollout_bench.py [--out profiles/r11_rollout.txt] [--steps 10] [--warmup 3] [--reps 5]

ViT-B/16, L = 12, precision fp16x3 (explicit: no error-word read per call), at B = 32 and B = 8 pairs of N = 500 patches and B = 4 pairs of
N = 5000.  Per shape it times, with HIP events around `steps` back-to-back calls after `warmup` calls, `reps` repetitions with the variants
interleaved inside each repetition (min-to-max spread stated):
    rollout    forward_rollout: scores, rollout (2, B, S) and last_attention (2, B, h, S) in one call
    forward    the unchanged forward at the same shape
    old_route  what the parent commit offers for the same answer: forward, two forward_vit(return_attention=True) (one per side, L maps of
               (B, h, S, S) fp32 each) and the rollout of the maps in torch on the device -- where the maps fit in memory
and reports the extra workspace a rollout call holds (rollout_workspace_bytes) beside workspace_bytes.  No bar is set: the numbers are
recorded as they come out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vtamiq_amd import VTAMIQ, synth  # noqa: E402

DEV = "cuda"
SHAPES = [(32, 500), (8, 500), (4, 5000)]


def make_model():
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", pretrained=False), precision="fp16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 0).items()})
    return m.to(DEV).eval()


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


def torch_rollout(maps, t):
    """e_t^T A_L ... A_1, A_l = (I + mean over heads of P_l) / 2, from L maps (B, h, S, S): what a user writes in torch."""
    B, _, S, _ = maps[0].shape
    r = torch.zeros(B, S, device=maps[0].device)
    r[:, t] = 1.0
    for P in reversed(maps):
        r = 0.5 * r + 0.5 * torch.einsum("bi,bij->bj", r, P.mean(1))
    return r


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))


def measure(model, B, N, a, lines, record):
    spec = model.spec
    pa, po, _ = synth.make_inputs(spec, B, N, 11)
    t = lambda x: torch.from_numpy(x).to(DEV)
    pr, pd, qr, qd = t(pa[:, 0]), t(pa[:, 1]), t(po[:, 0]), t(po[:, 1])
    inp = ((pr, pd), (qr, qd), (None, None))
    enc = model.transformer.encoder

    def old_route():
        q = model(*inp)[0]
        enc.return_attention = True
        try:
            out = []
            for p, ps in ((pr, qr), (pd, qd)):
                _, maps, _ = model.forward_vit(p, ps, None, tokens_only=True)
                out.append((torch_rollout(maps, 0), maps[-1][:, :, 0, :].clone()))
                del maps
        finally:
            enc.return_attention = False
        return q, torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])

    with torch.no_grad():
        variants = {"rollout": lambda: model.forward_rollout(*inp), "forward": lambda: model(*inp)}
        q, got = variants["rollout"]()
        q0 = variants["forward"]()[0]
        torch.cuda.synchronize()
        assert torch.equal(q.view(torch.int32), q0.view(torch.int32)) and bool(torch.isfinite(got.rollout).all())
        agree = "old route: the maps do not fit in memory"
        try:
            _, r_old, l_old = old_route()
            torch.cuda.synchronize()
            agree = (f"rollout vs old route: max abs difference {float((got.rollout - r_old).abs().max()):.2e}, "
                     f"last_attention {float((got.last_attention - l_old).abs().max()):.2e}")
            variants["old_route"] = old_route
            del r_old, l_old
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                heavy = k == "old_route"
                times[k].append(timed(fn, max(2, a.steps // 5) if heavy else a.steps, 1 if heavy else a.warmup))
    st = {k: stats(v) for k, v in times.items()}
    extra, base = model.rollout_workspace_bytes(B, N), model.workspace_bytes(B, N)
    S, h, L = N + spec.num_tokens, spec.num_heads, spec.num_layers
    lines.append(f"== B = {B}, N = {N} (S = {S}): ms per call, {a.reps} repetitions of {a.steps} steps behind {a.warmup} warm-ups (HIP events; old_route: "
                 f"{max(2, a.steps // 5)} steps behind 1), variants interleaved")
    lines.append(f"{'variant':<12}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}   repetitions")
    for k, s in st.items():
        lines.append(f"{k:<12}{s['median']:>10.3f}{s['min']:>10.3f}{s['max']:>10.3f}{s['spread']:>10.3f}   " + " ".join(f"{x:.3f}" for x in times[k]))
    f = st["forward"]["median"]
    lines.append(f"rollout / forward = {st['rollout']['median'] / f:.3f} (+{st['rollout']['median'] - f:.3f} ms)" +
                 (f";   old_route / forward = {st['old_route']['median'] / f:.3f};   old_route / rollout = "
                  f"{st['old_route']['median'] / st['rollout']['median']:.2f}" if "old_route" in st else ""))
    lines.append(agree)
    lines.append(f"workspace: forward {base / 2**20:.1f} MiB, rollout holds {extra / 2**20:.1f} MiB more; its outputs are {2 * B * S * (1 + h) * 4 / 2**10:.0f} KiB, "
                 f"the old route's maps {2 * L * B * h * S * S * 4 / 2**30:.2f} GiB ({L * B * h * S * S * 4 / 2**30:.2f} GiB alive at a time)")
    lines.append("")
    record[f"B{B}_N{N}"] = dict(times=st, rollout_workspace_bytes=extra, workspace_bytes=base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_rollout.txt"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/rollout_bench.py measures on the GPU: no device found")
    model = make_model()
    lines = [f"tools/rollout_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16, L = 12, precision fp16x3 (explicit)", ""]
    record = {}
    for B, N in SHAPES:
        measure(model, B, N, a, lines, record)
    lines.append("json: " + json.dumps(record))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
