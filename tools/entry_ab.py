#!/usr/bin/env python3
"""A/B of the engine's host code: does another build of the library compute and launch exactly what this one does?

    entry_ab.py hashes OUT.json [--config NAME ...] [--fp8]
        Every entry of tests/interleave.py's catalogue and every form of added_forms() on a fresh model, in every configuration below: the sha256 of each output tensor's
        bytes (or the text of the exception, where the call is refused), and vtq_workspace_bytes / vtq_rollout_workspace_bytes for the
        capacity the entry reserves.  --fp8 adds the fp8 experiment: forward_small twice on one VTAMIQFp8 (the calibrating call, then the
        next one), both scores and the chosen scales.  Run it once per library (VTQ_LIB_PATH / VTQ_LIB_PATH_FP8) and compare the files.
    entry_ab.py dispatches DIR_A DIR_B
        Two `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/entry_ab.py hashes ...` directories: the dispatch
        sequences as (kernel name, grid, workgroup size) in start order.  Prints the first difference, or "identical, n dispatches".

The tool only reads and prints; no test imports it."""
import argparse, csv, glob, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (precision, options, token); the option bits are _lib.OPT_FULL_LAST_LAYER = 1, _lib.OPT_FUSED_LAYERNORM = 4
CONFIGS = {
    "fp16x3": ("fp16x3", 0, 0), "bf16x3": ("bf16x3", 0, 0), "fp16x2": ("fp16x2", 0, 0), "fp16": ("fp16", 0, 0), "bf16": ("bf16", 0, 0),
    "fp16x3_full_last_layer": ("fp16x3", 1, 0), "bf16_full_last_layer": ("bf16", 1, 0), "fp16x3_fused_layernorm": ("fp16x3", 4, 0),
    "fp16x3_token1": ("fp16x3", 0, 1),
}
# the capacity each entry reserves: (sequence pairs, patches) -- ceil(sequences / 2) of its largest engine call, varlen its longest pair
CAPACITY = {
    "forward_small": (2, 40), "forward_large": (3, 300), "forward_rows_small": (2, 40), "pairwise_small": (3, 40), "pairwise_large": (3, 300),
    "vit_small": (2, 40), "vit_large": (3, 130), "rollout_small": (3, 40), "rollout_large": (3, 300), "varlen_small": (3, 130),
    "varlen_large": (4, 300), "group_small": (3, 40), "group_large": (3, 300), "cached_small": (2, 77),
}


# The forms the catalogue does not hold (`lengths=` on the one-to-many entries and on forward_rollout, `rollout=True`), on the same small
# model: G = 2 references, M = 3 distorted images; the ragged patch counts straddle the 128-row attention block edge, the uniform N is 40
LR, LD, LP, INDEX, N_UNIFORM = [5, 130], [130, 40, 5], [5, 130, 40], [1, 0, 1], 40


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def flat(x):
    """Every tensor of what a call returned, in order: tuples, Rollout fields and the list members of the ragged maps included."""
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in flat(y)]
    return [] if x is None else [x.rows] if hasattr(x, "rows") else [x]


def added_forms(il):
    """name -> ((sequence pairs, patches) the form reserves, call(model) -> what it returns)."""
    import numpy as np, torch
    from vtamiq_amd import synth
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(il.DEV)

    def ragged(lens, seed, image):                                   # one image list: patches (sum(lens), 3, P, P), pos (sum(lens), 2)
        pa, po, _ = synth.make_inputs(il.spec(), 1, sum(lens), seed)
        return dev(pa[0, image]), dev(po[0, image])
    r, d = {True: ragged(LR, 1201, 0)}, {True: ragged(LD, 1202, 1)}
    (p0, q0), (p1, q1) = ragged(LP, 1203, 0), ragged(LP, 1203, 1)
    u = il._group(2, 3, N_UNIFORM, INDEX)(1204)
    r[False], d[False] = (dev(u["p"][0]), dev(u["pos"][0])), (dev(u["p"][1]), dev(u["pos"][1]))

    def group(lengths, rollout):
        (pr, qr), (pd, qd), kw = r[lengths], d[lengths], dict(lengths=(LR, LD)) if lengths else {}
        return lambda m: m.forward_group((pr, pd), (qr, qd), None, INDEX, rollout=rollout, **kw)

    def cached(lengths, rollout):
        def call(m):
            ref = m.encode_reference(*r[lengths], None, lengths=LR if lengths else None, rollout=rollout)
            return ref, m.forward_cached(ref[0] if rollout else ref, *d[lengths], None, INDEX, lengths=LD if lengths else None, rollout=rollout)
        return call
    return {
        "group_lengths": ((3, 130), group(True, False)), "cached_lengths": ((2, 130), cached(True, False)),
        "rollout_lengths": ((3, 130), lambda m: m.forward_rollout((p0, p1), (q0, q1), None, lengths=LP)),
        "group_rollout": ((3, 40), group(False, True)), "cached_rollout": ((2, 40), cached(False, True)),
        "group_lengths_rollout": ((3, 130), group(True, True)), "cached_lengths_rollout": ((2, 130), cached(True, True)),
    }


def hashes(a):
    import torch
    from tests import interleave as il
    from vtamiq_amd import _lib
    assert set(CAPACITY) == set(il.CATALOGUE)
    out = {"library": {"abi": int(_lib.load().vtq_abi_version())}}
    forms = added_forms(il)
    for cname in a.config or CONFIGS:
        precision, options, token = CONFIGS[cname]
        m = il.build_model(precision, options, token)
        m._ensure_engine(torch.device(il.DEV))
        for name in il.CATALOGUE:
            B, N = CAPACITY[name]
            rec = {"workspace_bytes": m.workspace_bytes(B, N), "rollout_workspace_bytes": m.rollout_workspace_bytes(B, N)}
            try:
                rec["outputs"] = [sha(t) for t in il.fresh_outputs(name, precision, options, token)]
            except Exception as ex:                                  # a refusal: its text is part of the record
                rec["refused"] = f"{type(ex).__name__}: {ex}"
            out[f"{cname}/{name}"] = rec
        for name, ((B, N), call) in forms.items():
            rec = {"workspace_bytes": m.workspace_bytes(B, N), "rollout_workspace_bytes": m.rollout_workspace_bytes(B, N)}
            try:
                torch.cuda.synchronize()
                with torch.no_grad():
                    rec["outputs"] = [sha(t) for t in flat(call(il.build_model(precision, options, token)))]
            except Exception as ex:
                rec["refused"] = f"{type(ex).__name__}: {ex}"
            out[f"{cname}/{name}"] = rec
        del m
        print(f"{cname}: {len(il.CATALOGUE)} + {len(forms)} entries", flush=True)
    if a.fp8:
        from vtamiq_amd.experimental_fp8 import VTAMIQFp8
        m = VTAMIQFp8(**json.loads(json.dumps(il.KW)))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in il.state_dict().items()})
        m = m.to(il.DEV).eval()
        e = il.CATALOGUE["forward_small"]
        first = sha(e.run(m)[0])                                     # the calibrating call
        scales = m.fp8_scales()
        out["fp8/forward_small"] = {"calibrating": first, "next": sha(e.run(m)[0]), "scales": scales, "scales_after": m.fp8_scales()}
        print("fp8: forward_small twice", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {len(out) - 1} records, sha256 {hashlib.sha256(open(a.out, 'rb').read()).hexdigest()}")


def dispatch_list(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"{d}: no *kernel_trace.csv")
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    dim = lambda r, k: tuple(int(r[f"{k}_{ax}"]) for ax in "XYZ")
    return [(r["Kernel_Name"], dim(r, "Grid_Size"), dim(r, "Workgroup_Size")) for r in rows]


def dispatches(a):
    x, y = dispatch_list(a.dir_a), dispatch_list(a.dir_b)
    for i, (p, q) in enumerate(zip(x, y)):
        if p != q:
            print(f"dispatch {i} differs:\n  A {p}\n  B {q}")
            sys.exit(1)
    if len(x) != len(y):
        print(f"the first {min(len(x), len(y))} dispatches agree, then A has {len(x)} and B has {len(y)}")
        sys.exit(1)
    print(f"identical, {len(x)} dispatches")


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
sub = ap.add_subparsers(dest="cmd", required=True)
h = sub.add_parser("hashes")
h.add_argument("out")
h.add_argument("--config", nargs="+", choices=list(CONFIGS), help="these configurations only (default: all nine)")
h.add_argument("--fp8", action="store_true")
h.set_defaults(fn=hashes)
d = sub.add_parser("dispatches")
d.add_argument("dir_a")
d.add_argument("dir_b")
d.set_defaults(fn=dispatches)
a = ap.parse_args()
a.fn(a)
