#!/usr/bin/env python3
"""Micro-benchmark of forward_vit and its attention-probability kernel (GPU box).

  1. vtq_k_attention_probs alone at B = 32, S = 501, h = 12 and at B = 1, S = 5001: us per launch and the effective write rate
     B * h * S^2 * 4 bytes / time (the kernel is bound by that store stream; attention_probs.hip);
  2. VTAMIQ.forward_vit at B = 64 images, N = 500 (ViT-B/16, L = 12) with nothing / states / states + probs requested, next to the
     scoring forward at B = 32 pairs (the same 64 sequences plus the head).
HIP events around K launches after W warm-ups, median of 7 repeats (as tools/attn_bench.py)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tests.gpu_util import num_code, stream, to_planes
from vtamiq_amd import VTAMIQ, _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--fmt", nargs="+", default=["fp16x3", "bf16x3", "fp16", "bf16"])
ap.add_argument("--precision", nargs="+", default=["fp16x3", "fp16"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--json", default=None, help="also write the rows as JSON here")
a = ap.parse_args()
lib = _lib.load()
rows_out = []


def timed(call, reps=a.reps, warmup=a.warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    ts.sort()
    return ts[3] * 1e3, ts[0] * 1e3, ts[-1] * 1e3          # us: median, min, max


# ---- 1. the probabilities kernel alone ---------------------------------------------------------------------------------
H = 768
for nseq, S in ((32, 501), (1, 5001)):
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = (torch.randn(nseq * S, 3 * H, generator=g) * 0.5).cuda()
    out = torch.empty(nseq * 12 * S * S, device="cuda")
    nbytes = nseq * 12 * S * S * 4
    for fmt in a.fmt:
        P = to_planes(qkv, fmt, "a")
        q_log2 = int(fmt.endswith("x3"))
        call = lambda: _lib.check(lib.vtq_k_attention_probs(P.data_ptr(), P[0].numel(), out.data_ptr(), nseq, S, S, H, num_code(fmt), q_log2, stream()))
        med, lo, hi = timed(call)
        row = dict(kind="attention_probs", fmt=fmt, nseq=nseq, S=S, heads=12, us=med, us_min=lo, us_max=hi, bytes=nbytes,
                   write_tbps=nbytes / (med * 1e-6) / 1e12)
        rows_out.append(row)
        print(f"attention_probs {fmt:7s} nseq={nseq:3d} S={S}: {med:9.1f} us (min {lo:.1f}, max {hi:.1f})  {nbytes / 1e6:8.1f} MB  "
              f"{row['write_tbps']:.2f} TB/s effective write", flush=True)
        del P
    del qkv, out
    torch.cuda.empty_cache()

# ---- 2. forward_vit against the scoring forward ---------------------------------------------------------------------------
kw = dict(vit_config=dict(variant="ViT-B16", pretrained=False))
for prec in a.precision:
    m = VTAMIQ(**kw, precision=prec)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.spec, 5).items()})
    m = m.cuda().eval()
    patches, pos, _ = synth.make_inputs(m.spec, 32, 500, 4321)
    p = torch.from_numpy(patches).cuda()
    ps = torch.from_numpy(pos).cuda()
    pr, pd = p[:, 0].contiguous(), p[:, 1].contiguous()
    qr, qd = ps[:, 0].contiguous(), ps[:, 1].contiguous()
    imgs = torch.cat([pr, pd]).contiguous()                  # the same 64 sequences as single images
    pos64 = torch.cat([qr, qd]).contiguous()
    enc = m.transformer.encoder
    with torch.no_grad():
        med_fwd, lo, hi = timed(lambda: m((pr, pd), (qr, qd), (None, None)))
        print(f"{prec}: forward B=32 pairs (64 sequences + head): {med_fwd:9.1f} us", flush=True)
        rows_out.append(dict(kind="forward", precision=prec, pairs=32, us=med_fwd, us_min=lo, us_max=hi))
        for label, lay, att in (("nothing", False, False), ("states", True, False), ("states+probs", True, True)):
            enc.return_layers, enc.return_attention = lay, att
            med, lo, hi = timed(lambda: m.forward_vit(imgs, pos64, None, tokens_only=True), reps=2 if att else a.reps, warmup=1 if att else a.warmup)
            torch.cuda.empty_cache()
            print(f"{prec}: forward_vit B=64 images, {label:12s}: {med:9.1f} us  ({med / med_fwd:.3f} x the pair forward)", flush=True)
            rows_out.append(dict(kind="forward_vit", precision=prec, images=64, requested=label, us=med, us_min=lo, us_max=hi,
                                 ratio_to_forward=med / med_fwd))
    del m
    torch.cuda.empty_cache()

if a.json:
    with open(a.json, "w") as f:
        json.dump(rows_out, f, indent=1)
