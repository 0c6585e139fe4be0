"""Backward time with and without the gradients a caller can leave out (include/mdconv.h: MDCONV_FLAG_NO_GRAD_INPUT,
MDCONV_FLAG_NO_GRAD_WEIGHT).

    python tools/bench_selective_backward.py [--reps 30] [--rounds 5] [--shapes cfg2,cfg5_shard] [--plain-only]

Per shape the backward alone, through the caller-allocated C entry point in overwrite mode: four variants -- full,
no_weight, no_input, offsets_only (both flags) -- interleaved in one process, `rounds` measurements of `reps` calls between
two events each, after a warm-up per shape.  Prints one JSON line per (shape, variant) with the median and the spread over
the rounds.  MDCONV_LIB=<another build> with --plain-only measures that build's full backward on the same box (a build
from before the flags refuses them)."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from modulated_deform_conv_amd import MDCONV_CUDA as M, _capi

SHAPES = {
    # cfg2, its fp16 twin at B = 32 and B = 8, the cfg3 shard, cfg4 and the cfg5 shard (bench.py WORKLOADS)
    "cfg2": dict(nd=2, mod=True, B=32, C=256, O=256, sp=(56, 56), G=1, DG=1, dil=1, dtype=torch.float32, bias=True),
    "cfg2_fp16_b32": dict(nd=2, mod=True, B=32, C=256, O=256, sp=(56, 56), G=1, DG=1, dil=1, dtype=torch.float16, bias=True),
    "cfg2_fp16_b8": dict(nd=2, mod=True, B=8, C=256, O=256, sp=(56, 56), G=1, DG=1, dil=1, dtype=torch.float16, bias=True),
    "cfg3_shard": dict(nd=2, mod=True, B=32, C=256, O=256, sp=(56, 56), G=32, DG=4, dil=1, dtype=torch.float16, bias=False),
    "cfg4": dict(nd=3, mod=False, B=8, C=64, O=64, sp=(32, 32, 32), G=1, DG=1, dil=1, dtype=torch.float32, bias=False),
    "cfg5_shard": dict(nd=3, mod=True, B=8, C=128, O=128, sp=(16, 64, 64), G=1, DG=1, dil=2, dtype=torch.float16, bias=False),
}
VARIANTS = {"full": 0, "no_weight": _capi.FLAG_NO_GRAD_WEIGHT, "no_input": _capi.FLAG_NO_GRAD_INPUT,
            "offsets_only": _capi.FLAG_NO_GRAD_INPUT | _capi.FLAG_NO_GRAD_WEIGHT}


def setup(s):
    """-> {variant: callable}, tensors (kept alive by the caller)"""
    g = torch.Generator(device="cuda").manual_seed(0)
    dt, nd, mod = s["dtype"], s["nd"], s["mod"]
    r = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    B, C, O, G, DG, sp, dil = (s[k] for k in ("B", "C", "O", "G", "DG", "sp", "dil"))
    K = 3 ** nd
    x, off = r(B, C, *sp).to(dt), r(B, DG * nd * K, *sp).to(dt)
    m = torch.sigmoid(r(B, DG * K, *sp)).to(dt) if mod else None
    w, go = (r(O, C // G, *(3,) * nd) / math.sqrt(C // G * K)).to(dt), r(B, O, *sp).to(dt)
    b = (r(O) * 0.1).to(dt) if s["bias"] else x.new_empty(0)
    gi, goff, gw, gb = torch.empty_like(x), torch.empty_like(off), torch.empty_like(w), torch.empty_like(b)
    gm = torch.empty_like(m) if mod else None
    k3, one, pad, dl = (3,) * nd, (1,) * nd, (dil,) * nd, (dil,) * nd
    fns = {}
    for name, flags in VARIANTS.items():
        d = M._desc(nd, mod, x, w, k3, one, pad, dl, G, DG, 64, s["bias"])
        M._backward_checks(x, w, off, m, gi, gw, gb, goff, gm, go, d, s["bias"])
        d.accumulate = 0
        d.flags = flags
        if nd == 2 and mod:
            order = (x, w, b, off, m, go, gi, goff, gm, gw, gb)
        elif mod:
            order = (x, w, b, off, m, gi, gw, gb, goff, gm, go)
        else:
            order = (x, w, b, off, gi, gw, gb, goff, go)
        entry = "mdconv_%sdeform_conv%dd_backward" % ("modulated_" if mod else "", nd)
        args = [M._ptr(t) for t in order]
        fns[name] = (lambda d=d, args=args, entry=entry: M._run(entry, d, True, args, x))
    return fns, (x, w, b, off, m, go, gi, goff, gm, gw, gb)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        fns, keep = setup(SHAPES[name])
        if a.plain_only:
            fns = {"full": fns["full"]}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, a.reps))
        for k, v in ms.items():
            print(json.dumps(dict(shape=name, variant=k, lib=os.path.relpath(_capi.LIB_PATH), kernels=_capi.last_kernels(),
                                  median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))),
                  flush=True)
        del fns, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
