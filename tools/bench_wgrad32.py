"""Backward time of a 16-bit layer with and without fp32 weight gradients (include/mdconv.h: MDCONV_WGRAD_F32).

    python tools/bench_wgrad32.py [--reps 30] [--rounds 5]

Two shapes: the fp16 256 -> 256, 56 x 56, B = 8 layer and the cfg3 shard (bench.py WORKLOADS: 256 -> 256, 56 x 56, B = 32,
32 conv groups, 4 deformable groups, fp16, no bias).  Per shape the backward of the caller-allocated entry point in overwrite
mode, `rounds` interleaved measurements of `reps` calls each; prints one JSON line per (shape, mode) with the median and the
spread over the rounds.  MDCONV_LIB=<another build> measures that build's plain call (it has no fp32 mode: --plain-only)."""
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
    "fp16_256x256_56x56_b8": dict(B=8, C=256, O=256, H=56, W=56, G=1, DG=1, bias=True),
    "cfg3_shard": dict(B=32, C=256, O=256, H=56, W=56, G=32, DG=4, bias=False),
}


def setup(s, wdtype):
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    B, C, O, H, W, G, DG = (s[k] for k in ("B", "C", "O", "H", "W", "G", "DG"))
    x, off, m = r(B, C, H, W).half(), r(B, DG * 18, H, W).half(), torch.sigmoid(r(B, DG * 9, H, W)).half()
    w, go = (r(O, C // G, 3, 3) / math.sqrt(C // G * 9)).half(), r(B, O, H, W).half()
    b = (r(O) * 0.1).half() if s["bias"] else x.new_empty(0)
    gi, goff, gm = torch.empty_like(x), torch.empty_like(off), torch.empty_like(m)
    gw, gb = torch.empty_like(w, dtype=wdtype), torch.empty_like(b, dtype=wdtype)
    geo = (3, 3, 1, 1, 1, 1, 1, 1, G, DG, 64, s["bias"])
    d = M._desc(2, True, x, w, (3, 3), (1, 1), (1, 1), (1, 1), G, DG, 64, s["bias"])
    M._backward_checks(x, w, off, m, gi, gw, gb, goff, gm, go, d, s["bias"])
    d.accumulate = 0
    args = [M._ptr(t) for t in (x, w, b, off, m, go, gi, goff, gm, gw, gb)]
    return (lambda: M._run("mdconv_modulated_deform_conv2d_backward", d, True, args, x)), (x, w, b, off, m, go, gi, goff, gm, gw, gb)


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
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    for name, s in SHAPES.items():
        modes = {"plain": torch.float16} if a.plain_only else {"plain": torch.float16, "wgrad_f32": torch.float32}
        fns = {k: setup(s, v) for k, v in modes.items()}
        for fn, _ in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, (fn, _) in fns.items():
                ms[k].append(timed(fn, a.reps))
        for k, v in ms.items():
            print(json.dumps(dict(shape=name, mode=k, lib=os.path.basename(_capi.LIB_PATH), kernels=_capi.last_kernels(),
                                  median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))))


if __name__ == "__main__":
    main()
