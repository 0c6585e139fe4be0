"""What a channels-last 16-bit model pays around a deformable layer, with and without channels-last results
(include/mdconv.h: MDCONV_FLAG_OUTPUT_CHANNELS_LAST / MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST).

    python tools/bench_channels_last.py [--reps 20] [--rounds 7] [--shapes cfg2_fp16_b8,...] [--plain-only]

Per layer forward + backward through the C entry points (backward in overwrite mode) with a channels-last `input`, three
variants interleaved in one process:
  plain    the unflagged calls alone: contiguous output, grad_output and grad_input;
  a_today  the layer as a channels-last model runs it without the flags: the unflagged calls plus the three conversions that
           happen outside the library -- output.contiguous(memory_format=channels_last) by the next operator,
           grad_output.contiguous() on the way in, grad_input converted back to channels-last by the producer's backward;
  b_flags  the flagged calls: channels-last output, grad_output and grad_input, no conversion outside.
`rounds` measurements of `reps` steps between two events each, after a warm-up per variant; one JSON line per (layer,
variant) with the median and the spread (min, max) over the rounds.  MDCONV_LIB=<another build> with --plain-only measures
that build's unflagged calls on the same box (a build from before the flags refuses them)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from modulated_deform_conv_amd import MDCONV_CUDA as M, _capi

SHAPES = {
    # the fp16 twin of the headline layer at B = 8 and B = 32, the cfg3 and cfg5 shards (bench.py WORKLOADS), a 3-D 64 -> 64 layer
    "cfg2_fp16_b8": dict(nd=2, mod=True, B=8, C=256, O=256, sp=(56, 56), G=1, DG=1, dil=1, dtype=torch.float16, bias=True),
    "cfg2_fp16_b32": dict(nd=2, mod=True, B=32, C=256, O=256, sp=(56, 56), G=1, DG=1, dil=1, dtype=torch.float16, bias=True),
    "cfg3_shard": dict(nd=2, mod=True, B=32, C=256, O=256, sp=(56, 56), G=32, DG=4, dil=1, dtype=torch.float16, bias=False),
    "cfg5_shard": dict(nd=3, mod=True, B=8, C=128, O=128, sp=(16, 64, 64), G=1, DG=1, dil=2, dtype=torch.float16, bias=False),
    "dcn3d_c64_fp16": dict(nd=3, mod=False, B=8, C=64, O=64, sp=(16, 32, 32), G=1, DG=1, dil=1, dtype=torch.float16, bias=False),
}


def setup(s, plain_only):
    """-> {variant: callable running one forward + backward step}, the kernels' family, notes"""
    g = torch.Generator(device="cuda").manual_seed(0)
    dt, nd, mod = s["dtype"], s["nd"], s["mod"]
    fmt = torch.channels_last if nd == 2 else torch.channels_last_3d
    r = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    B, C, O, G, DG, sp, dil = (s[k] for k in ("B", "C", "O", "G", "DG", "sp", "dil"))
    K = 3 ** nd
    x = r(B, C, *sp).to(dt).contiguous(memory_format=fmt)
    off = r(B, DG * nd * K, *sp).to(dt)
    m = torch.sigmoid(r(B, DG * K, *sp)).to(dt) if mod else None
    w = (r(O, C // G, *(3,) * nd) / math.sqrt(C // G * K)).to(dt)
    b = (r(O) * 0.1).to(dt) if s["bias"] else x.new_empty(0)
    go = r(B, O, *sp).to(dt)
    go_cl = go.contiguous(memory_format=fmt)
    out, out_cl = torch.empty_like(go), torch.empty_like(go_cl)
    gi = torch.empty_like(x, memory_format=torch.contiguous_format)
    gi_cl = torch.empty_like(x)
    goff, gw, gb = torch.empty_like(off), torch.empty_like(w), torch.empty_like(b)
    gm = torch.empty_like(m) if mod else None
    k3, one, pad, dl = (3,) * nd, (1,) * nd, (dil,) * nd, (dil,) * nd
    notes = []

    def desc(flags, inp=None):
        d = M._desc(nd, mod, x, w, k3, one, pad, dl, G, DG, 64, s["bias"])
        d.accumulate = 0
        d.flags = flags
        d.input_layout = int(inp is not None and not inp.is_contiguous())
        return d

    def xin(backward):   # a channels-last input where this direction reads it in place, else the contiguous copy MDCONV_CUDA makes
        if _capi.lib().mdconv_input_layout_supported(ctypes.byref(desc(0)), 1, int(backward)):
            return x
        notes.append("%s: channels-last input not read in place" % ("backward" if backward else "forward"))
        return x.contiguous()

    xf, xb = xin(False), xin(True)
    name = "mdconv_%sdeform_conv%dd_" % ("modulated_" if mod else "", nd)

    def fwd(flags, o):
        args = [xf, w, b, off] + ([m] if mod else []) + [o]
        d = desc(flags, xf)
        return lambda: M._run(name + "forward", d, False, [M._ptr(t) for t in args], xf)

    def bwd(flags, gout, gin):
        if nd == 2 and mod:
            order = (xb, w, b, off, m, gout, gin, goff, gm, gw, gb)
        elif mod:
            order = (xb, w, b, off, m, gin, gw, gb, goff, gm, gout)
        else:
            order = (xb, w, b, off, gin, gw, gb, goff, gout)
        d = desc(flags, xb)
        return lambda: M._run(name + "backward", d, True, [M._ptr(t) for t in order], xb)

    f0, b0 = fwd(0, out), bwd(0, go, gi)

    def plain():
        f0()
        b0()

    def a_today():
        f0()
        out.contiguous(memory_format=fmt)      # the next operator's conversion
        go_cl.contiguous()                     # the incoming channels-last grad_output, made contiguous for the call
        b0()
        gi.contiguous(memory_format=fmt)       # grad_input back to the producer's layout

    fns = {"plain": plain}
    if not plain_only:
        flags = _capi.FLAG_OUTPUT_CHANNELS_LAST | _capi.FLAG_GRAD_INPUT_CHANNELS_LAST
        L = _capi.lib()
        ok = [bool(L.mdconv_result_layout_supported(ctypes.byref(desc(flags, xb if bw else xf)), int(bw))) for bw in (False, True)]
        fns["a_today"] = a_today
        if all(ok):
            f1, b1 = fwd(_capi.FLAG_OUTPUT_CHANNELS_LAST, out_cl), bwd(flags, go_cl, gi_cl)

            def b_flags():
                f1()
                b1()

            fns["b_flags"] = b_flags
        else:
            notes.append("result layouts not honoured (forward %d, backward %d): %s" % (ok[0], ok[1], _capi.last_error()))
    keep = (x, xf, xb, off, m, w, b, go, go_cl, out, out_cl, gi, gi_cl, goff, gw, gb, gm)
    return fns, keep, notes


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        fns, keep, notes = setup(SHAPES[name], a.plain_only)
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        kernels = _capi.last_kernels()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, a.reps))
        for k, v in ms.items():
            print(json.dumps(dict(shape=name, variant=k, lib=os.path.relpath(_capi.LIB_PATH), kernels=kernels,
                                  median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                                  notes=notes)), flush=True)
        del fns, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
